"""BF16 (GGML type 30, NTK_DT_BF16 = 9) on the host: the F32 -> BF16 conversion in numpy (gguf.f32_to_bf16) and in C++ (csrc/engine/synth.cpp) against a
float64 round-to-nearest-even, the row size, the GGUF round trip through both readers, what nt_gguf_describe reports, and the refusal of a type nobody knows.
No GPU."""
import struct

import numpy as np
import pytest

from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G


def bf16_grid():
    """every finite bfloat16 value as float64, ascending (both zeros collapse into one 0.0), and its bit pattern"""
    bits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    with np.errstate(invalid="ignore"):   # (signalling NaN patterns among the 65536)
        vals = G.bf16_to_f32(bits).astype(np.float64)
    keep = np.isfinite(vals) & ~((bits == 0x8000))
    bits, vals = bits[keep], vals[keep]
    order = np.argsort(vals, kind="stable")
    return vals[order], bits[order]


def rne_reference(x):
    """float32 -> bfloat16 bits by searching the grid of bfloat16 values in float64: the nearest one, ties to the even bit pattern, overflow to infinity
    when x is at or beyond the midpoint between the largest finite value and 2^128; the sign of a zero result is x's."""
    vals, bits = bf16_grid()
    out = np.empty(x.shape, np.uint16)
    top = float(vals[-1])
    over = (top + 2.0 ** 128) / 2.0
    for i, v in enumerate(x.astype(np.float64)):
        sign = np.signbit(x[i])
        if np.isnan(v):
            out[i] = 0xFFFF   # (checked apart: any NaN)
        elif abs(v) >= over:
            out[i] = 0xFF80 if sign else 0x7F80
        else:
            j = int(np.searchsorted(vals, v))
            cand = [k for k in (j - 1, j) if 0 <= k < len(vals)]
            best = min(cand, key=lambda k: (abs(vals[k] - v), int(bits[k]) & 1))
            b = int(bits[best])
            if vals[best] == 0.0:
                b = 0x8000 if sign else 0x0000
            out[i] = b
    return out


def special_inputs():
    f = np.float32
    r = np.random.Generator(np.random.Philox(key=[20261020, 1]))
    ties = np.array([0x3F808000, 0x3F818000, 0x3F828000, 0xBF808000, 0xBF818000, 0x00008000, 0x00018000, 0x007F8000, 0x3F807FFF, 0x3F808001],
                    np.uint32).view(np.float32)                 # exactly half way (even / odd below), one bit either side, among subnormals too
    big = np.array([3.3895314e38, 3.3961775e38, 3.4e38, np.finfo(f).max, -np.finfo(f).max], f)   # largest finite bf16, the overflow midpoint, beyond it
    sub = np.array([1e-45, 9.1835e-41, 4.6e-41, 1.1754942e-38, -1.0e-40, 5.877e-39], f)          # F32 and BF16 subnormals: kept, not flushed
    zero_inf = np.array([0.0, -0.0, np.inf, -np.inf], f)
    rand = r.standard_normal(2000).astype(f) * f(3.0)
    rbits = r.integers(0, 2 ** 32, 3000, dtype=np.uint64).astype(np.uint32).view(np.float32)
    rbits = rbits[np.isfinite(rbits)]
    return np.concatenate([ties, big, sub, zero_inf, rand, rbits]).astype(f)


def test_numpy_conversion_is_round_to_nearest_even():
    x = special_inputs()
    got = G.f32_to_bf16(x)
    want = rne_reference(x)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, [(x[i], hex(got[i]), hex(want[i])) for i in bad[:5]]
    assert got[np.signbit(x) & (x == 0)].tolist() == [0x8000] and G.f32_to_bf16(np.float32([0.0]))[0] == 0
    assert G.f32_to_bf16(np.float32([1e-45]))[0] == 0 and G.f32_to_bf16(np.float32([9.1835e-41]))[0] == 1     # subnormals survive
    # widening is exact and the round trip is the identity on every bfloat16 pattern that is not a NaN
    allbits = np.arange(0x10000, dtype=np.uint32).astype(np.uint16)
    wide = G.bf16_to_f32(allbits)
    ok = ~np.isnan(wide)
    assert np.array_equal(G.f32_to_bf16(wide[ok]), allbits[ok])


def test_nan_stays_nan_with_the_quiet_bit():
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7F80FFFF, 0x7FFFFFFF, 0x7FBF0000], np.uint32).view(np.float32)
    got = G.f32_to_bf16(nans)
    assert np.isnan(G.bf16_to_f32(got)).all()
    assert ((got & 0x0040) != 0).all()
    assert ((got >> 15) == (nans.view(np.uint32) >> 31)).all()


def test_cpp_converter_gives_the_same_bits():
    """The C++ generator draws a tensor's F32 values from (seed, tensor name, element index) whatever the mix, so the BF16 tensor must be the numpy
    conversion of the F32 one -- matrices at three scales (projection, embedding, head)."""
    for name in ("blk.0.attn_q.weight", "blk.1.ffn_down.weight", "token_embd.weight", "output.weight"):
        f32 = E.synth_tensor(E.synth_spec("tiny", "F32"), name).view("<f4")
        bf = E.synth_tensor(E.synth_spec("tiny", "BF16"), name).view("<u2")
        assert f32.size == bf.size and np.abs(f32).max() > 0
        assert np.array_equal(bf, G.f32_to_bf16(f32)), name
        assert (bf != (f32.view(np.uint32) >> 16).astype(np.uint16)).any(), "truncation would pass too: no value rounded up"


def test_row_bytes():
    L = _lib.lib()
    assert G.DT_BF16 == 9 and G.GGML_BF16 == 30 and G.GGML_TO_DT[G.GGML_BF16] == G.DT_BF16
    assert G.NAME_TO_GGML["BF16"] == G.GGML_BF16 and G.DT_NAME[G.DT_BF16] == "BF16"
    for n in (0, 1, 7, 4096):
        assert L.ntk_row_bytes(G.DT_BF16, n) == 2 * n == G.row_bytes(G.GGML_BF16, n)
    assert L.ntk_row_bytes(G.DT_BF16, -1) == 0 and L.ntk_row_bytes(10, 8) == 0


@pytest.fixture(scope="module")
def bf16_file(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bf16") / "tiny_bf16.gguf")
    types = G.make_synthetic_llama(path, G.TINY, "BF16", seed=20261020)
    return path, types


def test_gguf_round_trip_through_both_readers(bf16_file, tmp_path):
    path, types = bf16_file
    assert types["blk.0.attn_q.weight"] == G.GGML_BF16 and types["token_embd.weight"] == G.GGML_BF16 and types["output.weight"] == G.GGML_BF16
    f = G.read_gguf(path)
    d = E.gguf_describe(path)
    by_name = {t["name"]: t for t in d["tensors"]}
    for name, ti in f.tensors.items():
        c = by_name[name]
        assert (c["ggml_type"], c["offset"], c["nbytes"], tuple(c["dims"])) == (ti.ggml_type, ti.offset, ti.nbytes, ti.dims)
        if name.endswith("norm.weight"):
            assert ti.ggml_type == G.GGML_F32 and c["type"] == "F32"          # norm vectors stay F32
        else:
            assert ti.ggml_type == G.GGML_BF16 and c["dtype"] == G.DT_BF16 and c["type"] == "BF16"
            n = ti.dims[0] * ti.dims[1]
            assert ti.nbytes == 2 * n and f.dtype(name) == G.DT_BF16
    # the raw bytes are the written words; f32() and dequantize() widen them exactly
    name = "blk.1.ffn_up.weight"
    raw = np.array(f.raw(name))
    wide = f.f32(name)
    assert wide.dtype == np.float32 and np.array_equal(wide.view(np.uint32), raw.view("<u2").astype(np.uint32) << 16)
    assert np.array_equal(G.dequantize(raw, G.GGML_BF16, wide.size), wide)
    assert np.array_equal(G.f32_to_bf16(wide), raw.view("<u2"))
    assert 0.5 / 16 < float(np.sqrt(np.mean(wide.astype(np.float64) ** 2))) < 2.0 / 16      # RMS ~ 1 / sqrt(256)
    # the F32 twin the oracle reads: same metadata, same values, every tensor F32
    twin = str(tmp_path / "twin.gguf")
    G.write_f32_twin(path, twin)
    t = G.read_gguf(twin)
    assert t.meta == f.meta and list(t.tensors) == list(f.tensors)
    for name in f.tensors:
        assert t.tensors[name].ggml_type == G.GGML_F32
        assert np.array_equal(t.f32(name), f.f32(name))
    assert E.gguf_describe(twin)["hidden_size"] == d["hidden_size"] == G.TINY.hidden
    f.close(); t.close()


def test_overrides_mix_bf16_into_a_quantised_model(tmp_path):
    path = str(tmp_path / "q8_bf16_up.gguf")
    types = G.make_synthetic_llama(path, G.TINY, "Q8_0", overrides={"ffn_up": "BF16"})
    by_name = {t["name"]: t["type"] for t in E.gguf_describe(path)["tensors"]}
    for i in range(G.TINY.layers):
        assert types["blk.%d.ffn_up.weight" % i] == G.GGML_BF16 and by_name["blk.%d.ffn_up.weight" % i] == "BF16"
        assert by_name["blk.%d.ffn_gate.weight" % i] == "Q8_0"


def test_the_cpp_generator_writes_a_bf16_file(tmp_path):
    path = str(tmp_path / "synth_bf16.gguf")
    E.synth_write_gguf(path, E.synth_spec("tiny", "BF16"), 2)
    f = G.read_gguf(path)
    assert f.tensors["blk.0.attn_q.weight"].ggml_type == G.GGML_BF16 and f.tensors["blk.0.attn_norm.weight"].ggml_type == G.GGML_F32
    assert np.array_equal(np.array(f.raw("blk.0.attn_q.weight")), E.synth_tensor(E.synth_spec("tiny", "BF16"), "blk.0.attn_q.weight"))
    assert {t["type"] for t in E.gguf_describe(path)["tensors"]} == {"BF16", "F32"}
    f.close()


def test_an_unknown_ggml_type_is_still_refused(bf16_file, tmp_path):
    """Type 30 became known; its neighbours did not.  The same file with one tensor's type word patched to 31: the numpy reader has no block size for it,
    and the C++ reader reports it as unknown (the loader refuses such a tensor: "Unsupported tensor type", tests/test_engine_unquantised_gpu.py)."""
    path, _ = bf16_file
    blob = bytearray(open(path, "rb").read())
    key = b"blk.0.attn_k.weight"
    at = blob.index(struct.pack("<Q", len(key)) + key) + 8 + len(key)
    nd = struct.unpack_from("<I", blob, at)[0]
    tpos = at + 4 + 8 * nd
    assert struct.unpack_from("<I", blob, tpos)[0] == G.GGML_BF16
    struct.pack_into("<I", blob, tpos, 31)
    bad = str(tmp_path / "type31.gguf")
    open(bad, "wb").write(bytes(blob))
    with pytest.raises(KeyError):
        G.read_gguf(bad)
    types = {t["name"]: t["type"] for t in E.gguf_describe(bad)["tensors"]}
    assert types["blk.0.attn_k.weight"] == "UNKNOWN" and types["blk.0.attn_q.weight"] == "BF16"
