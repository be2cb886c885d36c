"""GGUF v3 container: writer, reader and seeded synthetic Llama-shaped models (numpy only).

The reference can only *read* GGUF (reference src/model/loader.cpp:56-187); it ships no writer and no
model files exist in this environment, so every parity/bench input is a synthetic file produced here
(small fixtures, tests) or by the C++ generator in csrc/synth.cpp (8B/70B shapes, same container).

Layout facts this file must agree with the reference loader on:
  * header: magic "GGUF", version 3, n_tensors u64, n_kv u64                      (loader.cpp:60-83)
  * kv: key string, type u32, value; arrays = elem type u32 + count u64 + elems   (loader.cpp:91-131)
  * keys read: general.architecture/name/alignment, <arch>.{vocab_size, embedding_length,
    feed_forward_length, block_count, attention.head_count, attention.head_count_kv, context_length,
    attention.layer_norm_rms_epsilon, rope.freq_base}, tokenizer.ggml.{tokens, scores, token_type,
    bos_token_id, eos_token_id}                                  (reference src/model/config.cpp:24-49)
  * tensor info: name, n_dims u32, dims u64[n] in ggml order (fastest first = in_features first),
    ggml type u32, offset u64 relative to the aligned data section      (loader.cpp:146-170,177-185)
  * quant block byte layouts                                     (reference src/core/types.h:96-137)
"""
from __future__ import annotations

import mmap
import struct
from dataclasses import dataclass, field
from typing import Dict, Iterable, List, Optional, Sequence, Tuple

import numpy as np

GGUF_MAGIC = 0x46554747

# GGUF metadata value types (reference src/core/types.h:156-170)
T_U8, T_I8, T_U16, T_I16, T_U32, T_I32, T_F32, T_BOOL, T_STR, T_ARR, T_U64, T_I64, T_F64 = range(13)

# ggml tensor types the reference maps (types.h:173-215)
GGML_F32, GGML_F16, GGML_Q4_0, GGML_Q8_0, GGML_Q4_K, GGML_Q5_K, GGML_Q6_K = 0, 1, 2, 8, 12, 13, 14
GGML_BF16 = 30   # not in the reference: bfloat16, the format checkpoints are published in

# nt::DType numeric values (types.h:24-35) -- the C ABI contract
DT_F32, DT_F16, DT_Q8_0, DT_Q4_0, DT_Q4_K, DT_Q6_K, DT_Q5_K, DT_Q2_K, DT_I32 = range(9)
DT_BF16 = 9   # NTK_DT_BF16: appended behind the reference's values

GGML_TO_DT = {GGML_F32: DT_F32, GGML_F16: DT_F16, GGML_Q4_0: DT_Q4_0, GGML_Q8_0: DT_Q8_0,
              GGML_Q4_K: DT_Q4_K, GGML_Q5_K: DT_Q5_K, GGML_Q6_K: DT_Q6_K, GGML_BF16: DT_BF16}
DT_TO_GGML = {v: k for k, v in GGML_TO_DT.items()}
DT_NAME = {DT_F32: "F32", DT_F16: "F16", DT_Q8_0: "Q8_0", DT_Q4_0: "Q4_0", DT_Q4_K: "Q4_K",
           DT_Q6_K: "Q6_K", DT_Q5_K: "Q5_K", DT_BF16: "BF16"}
NAME_TO_GGML = {"F32": GGML_F32, "F16": GGML_F16, "Q4_0": GGML_Q4_0, "Q8_0": GGML_Q8_0,
                "Q4_K": GGML_Q4_K, "Q5_K": GGML_Q5_K, "Q6_K": GGML_Q6_K, "BF16": GGML_BF16}

# (elements per block, bytes per block)
BLOCK = {GGML_F32: (1, 4), GGML_F16: (1, 2), GGML_Q4_0: (32, 18), GGML_Q8_0: (32, 34),
         GGML_Q4_K: (256, 144), GGML_Q5_K: (256, 176), GGML_Q6_K: (256, 210), GGML_BF16: (1, 2)}


def f32_to_bf16(x: np.ndarray) -> np.ndarray:
    """float32 -> bfloat16 bit patterns (uint16, same shape): round to nearest even on the 16 dropped bits, subnormals kept (no flush), +-inf kept,
    NaN stays NaN with the quiet bit set (the rounding add could otherwise carry a NaN's payload into infinity)."""
    u = np.ascontiguousarray(x, dtype="<f4").view(np.uint32)
    rounded = (u + (np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1)))) >> np.uint32(16)
    nan = (u & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)
    return np.where(nan, (u >> np.uint32(16)) | np.uint32(0x0040), rounded).astype(np.uint16)


def bf16_to_f32(bits: np.ndarray) -> np.ndarray:
    """bfloat16 bit patterns -> float32: the bits become the high half, exactly."""
    return (np.ascontiguousarray(bits).view("<u2").astype(np.uint32) << np.uint32(16)).view("<f4")


def row_bytes(ggml_type: int, n: int) -> int:
    be, bb = BLOCK[ggml_type]
    assert n % be == 0, (ggml_type, n)
    return (n // be) * bb


# ----------------------------------------------------------------------------------------------
# writer
# ----------------------------------------------------------------------------------------------
def _s(b: bytes | str) -> bytes:
    if isinstance(b, str):
        b = b.encode("utf-8")
    return struct.pack("<Q", len(b)) + b


def _kv(key: str, vtype: int, payload: bytes) -> bytes:
    return _s(key) + struct.pack("<I", vtype) + payload


def kv_u32(key, v): return _kv(key, T_U32, struct.pack("<I", v))
def kv_f32(key, v): return _kv(key, T_F32, struct.pack("<f", v))
def kv_str(key, v): return _kv(key, T_STR, _s(v))


def kv_arr_str(key, items: Sequence[bytes | str]) -> bytes:
    body = b"".join(_s(x) for x in items)
    return _kv(key, T_ARR, struct.pack("<IQ", T_STR, len(items)) + body)


def kv_arr_i32(key, items: Sequence[int]) -> bytes:
    return _kv(key, T_ARR, struct.pack("<IQ", T_I32, len(items)) + np.asarray(items, "<i4").tobytes())


def kv_arr_f32(key, items: Sequence[float]) -> bytes:
    return _kv(key, T_ARR, struct.pack("<IQ", T_F32, len(items)) + np.asarray(items, "<f4").tobytes())


@dataclass
class TensorSpec:
    name: str
    dims: Tuple[int, ...]      # ggml order: (in_features, out_features) for matrices, (n,) for vectors
    ggml_type: int
    data: Optional[bytes] = None   # raw bytes; or a callable returning bytes (lazy, for big files)

    @property
    def nbytes(self) -> int:
        n = 1
        for d in self.dims:
            n *= d
        return row_bytes(self.ggml_type, n)


def write_gguf(path: str, kvs: Sequence[bytes], tensors: Sequence[TensorSpec], alignment: int = 32) -> None:
    """Write a GGUF v3 file. Tensor data is laid out in order, each tensor aligned to `alignment`."""
    header = struct.pack("<IIQQ", GGUF_MAGIC, 3, len(tensors), len(kvs)) + b"".join(kvs)
    infos = []
    off = 0
    offsets = []
    for t in tensors:
        offsets.append(off)
        infos.append(_s(t.name) + struct.pack("<I", len(t.dims)) + struct.pack("<%dQ" % len(t.dims), *t.dims)
                     + struct.pack("<IQ", t.ggml_type, off))
        off += (t.nbytes + alignment - 1) // alignment * alignment
    head = header + b"".join(infos)
    pad = (-len(head)) % alignment
    with open(path, "wb") as f:
        f.write(head + b"\0" * pad)
        for t, o in zip(tensors, offsets):
            data = t.data() if callable(t.data) else t.data
            assert data is not None and len(data) == t.nbytes, (t.name, len(data or b""), t.nbytes)
            f.write(data)
            f.write(b"\0" * ((-t.nbytes) % alignment))


# ----------------------------------------------------------------------------------------------
# reader (independent of the C++ loader; used by the oracle-side forward and by tests)
# ----------------------------------------------------------------------------------------------
@dataclass
class TensorInfo:
    name: str
    dims: Tuple[int, ...]
    ggml_type: int
    offset: int
    nbytes: int


@dataclass
class GGUFFile:
    path: str
    version: int
    meta: Dict[str, object]
    tensors: Dict[str, TensorInfo]
    data_offset: int
    _mm: Optional[mmap.mmap] = field(default=None, repr=False)
    _buf: Optional[np.ndarray] = field(default=None, repr=False)
    kv_span: Tuple[int, int] = (0, 0)   # file bytes [a, b) of the metadata entries, as written (write_f32_twin copies them)

    def raw(self, name: str) -> np.ndarray:
        ti = self.tensors[name]
        a = self.data_offset + ti.offset
        return self._buf[a:a + ti.nbytes]

    def dtype(self, name: str) -> int:
        return GGML_TO_DT[self.tensors[name].ggml_type]

    def f32(self, name: str) -> np.ndarray:
        if self.tensors[name].ggml_type == GGML_BF16:   # widened exactly (a copy: the file holds 16-bit words)
            return bf16_to_f32(self.raw(name).view("<u2"))
        assert self.tensors[name].ggml_type == GGML_F32
        return self.raw(name).view("<f4")

    def close(self):
        self._buf = None
        if self._mm is not None:
            self._mm.close()
            self._mm = None


def read_gguf(path: str) -> GGUFFile:
    f = open(path, "rb")
    mm = mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ)
    buf = np.frombuffer(mm, dtype=np.uint8)
    pos = 0

    def rd(fmt):
        nonlocal pos
        v = struct.unpack_from("<" + fmt, mm, pos)
        pos += struct.calcsize("<" + fmt)
        return v if len(v) > 1 else v[0]

    def rstr():
        nonlocal pos
        n = rd("Q")
        s = bytes(mm[pos:pos + n])
        pos += n
        return s

    scalar = {T_U8: "B", T_I8: "b", T_U16: "H", T_I16: "h", T_U32: "I", T_I32: "i", T_F32: "f",
              T_BOOL: "?", T_U64: "Q", T_I64: "q", T_F64: "d"}

    def rval(t):
        if t == T_STR:
            return rstr()
        if t == T_ARR:
            et, n = rd("I"), rd("Q")
            return [rval(et) for _ in range(n)]
        return rd(scalar[t])

    magic, version = rd("I"), rd("I")
    if magic != GGUF_MAGIC:
        raise ValueError("bad GGUF magic 0x%08x" % magic)
    if version not in (2, 3):
        raise ValueError("unsupported GGUF version %d" % version)
    n_tensors, n_kv = rd("Q"), rd("Q")
    meta: Dict[str, object] = {}
    kv_begin = pos
    for _ in range(n_kv):
        k = rstr().decode("utf-8")
        t = rd("I")
        meta[k] = rval(t)
    kv_end = pos
    tensors: Dict[str, TensorInfo] = {}
    for _ in range(n_tensors):
        name = rstr().decode("utf-8")
        nd = rd("I")
        dims = tuple(rd("Q") for _ in range(nd))
        gt, off = rd("I"), rd("Q")
        n = 1
        for d in dims:
            n *= d
        tensors[name] = TensorInfo(name, dims, gt, off, row_bytes(gt, n))
    align = int(meta.get("general.alignment", 32))
    data_offset = (pos + align - 1) // align * align
    return GGUFFile(path, version, meta, tensors, data_offset, mm, buf, (kv_begin, kv_end))


def write_f32_twin(src: str, dst: str, widen: Sequence[int] = (GGML_BF16,)) -> None:
    """`src` again with every tensor whose type is in `widen` stored as F32 holding the same VALUES (exact: a bfloat16 or half value is a float), the
    other tensors and the metadata copied byte for byte: the file a reader without BF16 -- the oracle -- computes the model's reference from, with no
    quantiser in between."""
    f = read_gguf(src)
    n_kv = len(f.meta)
    kvs = [bytes(f._buf[f.kv_span[0]:f.kv_span[1]])] + [b""] * (n_kv - 1)   # (write_gguf counts the entries and joins them)
    specs = []
    for name, ti in f.tensors.items():
        n = 1
        for d in ti.dims:
            n *= d
        if ti.ggml_type in widen:
            specs.append(TensorSpec(name, ti.dims, GGML_F32, dequantize(np.array(f.raw(name)), ti.ggml_type, n).astype("<f4").tobytes()))
        else:
            specs.append(TensorSpec(name, ti.dims, ti.ggml_type, bytes(f.raw(name))))
    f.close()
    write_gguf(dst, kvs, specs)


# ----------------------------------------------------------------------------------------------
# synthetic quantised tensors (blocks generated directly)
# ----------------------------------------------------------------------------------------------
def _f16_bytes(x: np.ndarray) -> np.ndarray:
    return x.astype("<f2").view(np.uint8).reshape(x.shape + (2,))


def synth_tensor(rng: np.random.Generator, ggml_type: int, out_f: int, in_f: int, sigma: float = 1.0) -> bytes:
    """Random [out_f, in_f] matrix in `ggml_type` encoding with dequantised RMS ~ sigma/sqrt(in_f)."""
    be, bb = BLOCK[ggml_type]
    nb = out_f * in_f // be
    tgt = sigma / np.sqrt(in_f)
    jit = (1.0 + 0.25 * rng.uniform(-1, 1, nb)).astype(np.float32)
    if ggml_type == GGML_F32:
        return (rng.standard_normal(out_f * in_f) * tgt).astype("<f4").tobytes()
    if ggml_type == GGML_F16:
        return (rng.standard_normal(out_f * in_f) * tgt).astype("<f2").tobytes()
    if ggml_type == GGML_BF16:
        return f32_to_bf16((rng.standard_normal(out_f * in_f) * tgt).astype("<f4")).astype("<u2").tobytes()
    blk = np.empty((nb, bb), np.uint8)
    if ggml_type == GGML_Q8_0:
        blk[:, 0:2] = _f16_bytes(tgt / 73.3 * jit)
        blk[:, 2:] = rng.integers(-127, 128, (nb, 32), dtype=np.int8).view(np.uint8)
    elif ggml_type == GGML_Q4_0:
        blk[:, 0:2] = _f16_bytes(tgt / 4.6 * jit)
        blk[:, 2:] = rng.integers(0, 256, (nb, 16), dtype=np.uint8)
    elif ggml_type in (GGML_Q4_K, GGML_Q5_K):
        mean_q = 7.5 if ggml_type == GGML_Q4_K else 15.5
        dev_q = 4.6 if ggml_type == GGML_Q4_K else 9.2
        d = tgt / (32.0 * dev_q * 1.6) * jit
        blk[:, 0:2] = _f16_bytes(d)
        blk[:, 2:4] = _f16_bytes(d * mean_q)             # dmin*m ~ d*sc*mean(q): roughly centred
        blk[:, 4:16] = rng.integers(0, 256, (nb, 12), dtype=np.uint8)
        blk[:, 16:] = rng.integers(0, 256, (nb, bb - 16), dtype=np.uint8)
    elif ggml_type == GGML_Q6_K:
        blk[:, 0:192] = rng.integers(0, 256, (nb, 192), dtype=np.uint8)
        blk[:, 192:208] = rng.integers(-64, 64, (nb, 16), dtype=np.int8).view(np.uint8)
        blk[:, 208:210] = _f16_bytes(tgt / (37.0 * 18.5) * jit)
    else:
        raise ValueError(ggml_type)
    return blk.tobytes()


# ----------------------------------------------------------------------------------------------
# dequantisation (numpy, written from the block definitions in SURVEY Appendix A; an independent
# statement used to cross-check the oracle, the HIP embedding gather and the golden fixtures)
# ----------------------------------------------------------------------------------------------
def _kq_scales(sc: np.ndarray):
    """sc: [nb, 12] uint8 -> (scale[nb,8], min[nb,8]) 6-bit values."""
    sc = sc.astype(np.int32)
    s = np.empty(sc.shape[:-1] + (8,), np.int32)
    m = np.empty_like(s)
    s[..., :4] = sc[..., 0:4] & 63
    m[..., :4] = sc[..., 4:8] & 63
    s[..., 4:] = (sc[..., 8:12] & 0xF) | ((sc[..., 0:4] >> 6) << 4)
    m[..., 4:] = (sc[..., 8:12] >> 4) | ((sc[..., 4:8] >> 6) << 4)
    return s, m


def dequantize(raw: np.ndarray | bytes, ggml_type: int, n: int) -> np.ndarray:
    """raw bytes of n elements -> float32[n] (same element order as the row)."""
    raw = np.frombuffer(raw, np.uint8) if not isinstance(raw, np.ndarray) else raw.view(np.uint8).reshape(-1)
    be, bb = BLOCK[ggml_type]
    nb = n // be
    if ggml_type == GGML_F32:
        return raw.view("<f4").astype(np.float32)
    if ggml_type == GGML_F16:
        return raw.view("<f2").astype(np.float32)
    if ggml_type == GGML_BF16:
        return bf16_to_f32(raw[: 2 * n].view("<u2"))
    b = raw[: nb * bb].reshape(nb, bb)
    if ggml_type == GGML_Q8_0:
        d = b[:, 0:2].copy().view("<f2").astype(np.float32)
        return (d * b[:, 2:].view(np.int8).astype(np.float32)).reshape(-1)
    if ggml_type == GGML_Q4_0:
        d = b[:, 0:2].copy().view("<f2").astype(np.float32)
        q = b[:, 2:]
        lo = (q & 0xF).astype(np.float32) - 8
        hi = (q >> 4).astype(np.float32) - 8
        return (d * np.concatenate([lo, hi], 1)).reshape(-1)
    if ggml_type in (GGML_Q4_K, GGML_Q5_K):
        d = b[:, 0:2].copy().view("<f2").astype(np.float32)
        dm = b[:, 2:4].copy().view("<f2").astype(np.float32)
        s, m = _kq_scales(b[:, 4:16])
        if ggml_type == GGML_Q4_K:
            qs = b[:, 16:144].reshape(nb, 4, 32)
            lo = (qs & 0xF).astype(np.float32)
            hi = (qs >> 4).astype(np.float32)
        else:
            qh = b[:, 16:48].astype(np.int32)[:, None, :]
            ql = b[:, 48:176].reshape(nb, 4, 32).astype(np.int32)
            c = np.arange(4)[None, :, None]
            lo = ((ql & 0xF) + (((qh >> (2 * c)) & 1) << 4)).astype(np.float32)
            hi = ((ql >> 4) + (((qh >> (2 * c + 1)) & 1) << 4)).astype(np.float32)
        q = np.stack([lo, hi], 2).reshape(nb, 8, 32)         # sub-block order 0..7
        w = (d * s.astype(np.float32))[:, :, None] * q - (dm * m.astype(np.float32))[:, :, None]
        return w.reshape(-1).astype(np.float32)
    if ggml_type == GGML_Q6_K:
        ql = b[:, 0:128].reshape(nb, 2, 64).astype(np.int32)
        qh = b[:, 128:192].reshape(nb, 2, 32).astype(np.int32)
        sc = b[:, 192:208].view(np.int8).reshape(nb, 2, 8).astype(np.float32)
        d = b[:, 208:210].copy().view("<f2").astype(np.float32)
        q1 = ((ql[:, :, :32] & 0xF) | (((qh >> 0) & 3) << 4)) - 32
        q2 = ((ql[:, :, 32:] & 0xF) | (((qh >> 2) & 3) << 4)) - 32
        q3 = ((ql[:, :, :32] >> 4) | (((qh >> 4) & 3) << 4)) - 32
        q4 = ((ql[:, :, 32:] >> 4) | (((qh >> 6) & 3) << 4)) - 32
        q = np.stack([q1, q2, q3, q4], 2).astype(np.float32)          # [nb, 2, 4, 32]
        isx = np.arange(32) // 16
        scl = np.stack([sc[:, :, isx + 2 * g] for g in range(4)], 2)  # [nb, 2, 4, 32]
        w = d[:, :, None, None] * scl * q
        return w.reshape(-1).astype(np.float32)
    raise ValueError(ggml_type)


# ----------------------------------------------------------------------------------------------
# synthetic Llama-shaped models
# ----------------------------------------------------------------------------------------------
@dataclass
class LlamaShape:
    name: str
    hidden: int
    inter: int
    layers: int
    heads: int
    kv_heads: int
    vocab: int
    ctx: int = 131072
    eps: float = 1e-5
    theta: float = 500000.0
    bos: int = 1
    eos: int = 2
    head_dim: int = 0     # 0: hidden / heads; else a head size of its own, written as <arch>.attention.key_length / value_length

    @property
    def hd(self) -> int:
        return self.head_dim or self.hidden // self.heads


TINY = LlamaShape("tiny", 256, 512, 2, 4, 2, 512, ctx=256, bos=256, eos=257)
SMALL = LlamaShape("small", 1024, 2048, 4, 8, 2, 2048, ctx=2048, bos=256, eos=257)       # hd=128, GQA 4
LLAMA_8B = LlamaShape("llama3.1-8b", 4096, 14336, 32, 32, 8, 128256, bos=128000, eos=128009)
LLAMA_70B = LlamaShape("llama3.1-70b", 8192, 28672, 80, 64, 8, 128256, bos=128000, eos=128009)
# Qwen2 (make_synthetic_llama(..., arch="qwen2", qkv_bias=<scale>)): the published geometry, and the two-layer shapes of the engine tests
QWEN25_7B = LlamaShape("qwen2.5-7b", 3584, 18944, 28, 28, 4, 152064, ctx=32768, eps=1e-6, theta=1e6, bos=151643, eos=151645)
QWEN_T64 = LlamaShape("qt64", 256, 512, 2, 4, 2, 512, ctx=1024, eps=1e-6, theta=1e6, bos=256, eos=257)        # the TINY shape: head_dim 64
QWEN_T128 = LlamaShape("qt128", 256, 512, 2, 2, 1, 512, ctx=1024, eps=1e-6, theta=1e6, bos=256, eos=257)      # head_dim 128
QWEN_7 = LlamaShape("q7", 1792, 512, 2, 14, 2, 512, ctx=1024, eps=1e-6, theta=1e6, bos=256, eos=257)          # head_dim 128, 7 query heads per KV head (Qwen2.5-7B's ratio)
# Qwen3 (make_synthetic_llama(..., arch="qwen3", qk_norm=<scale>)): the published geometries -- Qwen3-4B's 32 heads of 128 over a hidden size of 2560 --
# and the two-layer shapes of the engine tests; NEMO_128: Mistral-Nemo's kind under `llama`, heads x head_dim BELOW the hidden size and no norm tensors
QWEN3_8B = LlamaShape("qwen3-8b", 4096, 12288, 36, 32, 8, 151936, ctx=40960, eps=1e-6, theta=1e6, bos=151643, eos=151645, head_dim=128)
QWEN3_4B = LlamaShape("qwen3-4b", 2560, 9728, 36, 32, 8, 151936, ctx=40960, eps=1e-6, theta=1e6, bos=151643, eos=151645, head_dim=128)
QWEN3_N64 = LlamaShape("q3n64", 256, 512, 2, 4, 2, 512, ctx=1024, eps=1e-6, theta=1e6, bos=256, eos=257)                   # head_dim 64 = hidden / heads
QWEN3_W128 = LlamaShape("q3w128", 256, 512, 2, 4, 2, 512, ctx=1024, eps=1e-6, theta=1e6, bos=256, eos=257, head_dim=128)   # 4 x 128 = 512 > hidden
QWEN3_G128 = LlamaShape("q3g128", 1024, 512, 2, 8, 2, 512, ctx=1024, eps=1e-6, theta=1e6, bos=256, eos=257)               # head_dim 128, 4 query heads per KV head
NEMO_128 = LlamaShape("nemo128", 512, 512, 2, 2, 1, 512, ctx=1024, eps=1e-6, theta=1e6, bos=256, eos=257, head_dim=128)    # 2 x 128 = 256 < hidden


# Mixture-of-experts (make_synthetic_llama(..., experts=E, experts_used=K, expert_inter=I_e)): the published geometries and the two-layer shapes of the
# engine tests.  Qwen3-30B-A3B: 128 experts of width 768, 8 per token; Mixtral 8x7B (architecture `llama`): 8 experts of width 14336, 2 per token
QWEN3_30B_A3B = LlamaShape("qwen3-30b-a3b", 2048, 6144, 48, 32, 4, 151936, ctx=40960, eps=1e-6, theta=1e6, bos=151643, eos=151645, head_dim=128)
MIXTRAL_8X7B = LlamaShape("mixtral-8x7b", 4096, 14336, 32, 32, 8, 32000, ctx=32768, eps=1e-5, theta=1e6, bos=1, eos=2)
MOE_8Q8 = LlamaShape("moe8q8", 256, 512, 2, 4, 2, 512, ctx=1024, eps=1e-6, theta=1e6, bos=256, eos=257)                    # heads of 64
MOE_4K = LlamaShape("moe4k", 256, 512, 2, 4, 2, 512, ctx=1024, eps=1e-6, theta=1e6, bos=256, eos=257, head_dim=128)        # heads of 128, key_length
MIXTRAL_4 = LlamaShape("mixtral4", 512, 256, 2, 4, 2, 512, ctx=1024, eps=1e-5, theta=1e6, bos=256, eos=257)                # I_e = feed_forward_length


def model_head_dim(meta: Dict[str, object]) -> int:
    """The head size a file's metadata states: <arch>.attention.key_length where the key is there (Qwen3, Mistral-Nemo), else embedding_length / head_count.
    ValueError names the key when key_length is not a positive even number or value_length differs from it (the engine refuses the same files)."""
    arch = meta.get("general.architecture", b"llama")
    arch = arch.decode() if isinstance(arch, bytes) else arch
    kname, vname = arch + ".attention.key_length", arch + ".attention.value_length"
    if kname not in meta:
        return int(meta[arch + ".embedding_length"]) // int(meta[arch + ".attention.head_count"])
    hd = int(meta[kname])
    if hd <= 0 or hd % 2:
        raise ValueError("%s = %d: the head size must be positive and even" % (kname, hd))
    if vname in meta and int(meta[vname]) != hd:
        raise ValueError("%s = %d differs from %s = %d" % (vname, int(meta[vname]), kname, hd))
    return hd


def use_more_bits(i: int, n: int) -> bool:
    """llama.cpp's Q4_K_M rule."""
    return i < n // 8 or i >= 7 * n // 8 or (i - n // 8) % 3 == 2


def tensor_types(shape: LlamaShape, mix: str) -> Dict[str, int]:
    """name -> ggml type for a quantisation mix: a plain type name or 'Q4_K_M'."""
    L = shape.layers
    out: Dict[str, int] = {}
    mats = ["attn_q", "attn_k", "attn_v", "attn_output", "ffn_gate", "ffn_up", "ffn_down"]
    if mix == "Q4_K_M":
        gqa = shape.heads // shape.kv_heads
        out["token_embd.weight"] = GGML_Q4_K
        out["output.weight"] = GGML_Q6_K
        for i in range(L):
            for m in mats:
                t = GGML_Q4_K
                if m in ("attn_v", "ffn_down") and use_more_bits(i, L):
                    t = GGML_Q6_K
                elif m == "attn_v" and gqa >= 4 and shape.hidden >= 8192:
                    t = GGML_Q5_K  # 70B-class GQA: remaining attn_v -> Q5_K
                out["blk.%d.%s.weight" % (i, m)] = t
    elif mix == "MIXED":  # every quant type in one small file (tests)
        cyc = [GGML_Q8_0, GGML_Q4_0, GGML_Q4_K, GGML_Q5_K, GGML_Q6_K, GGML_F16, GGML_F32]
        out["token_embd.weight"] = GGML_Q4_K
        out["output.weight"] = GGML_Q6_K
        k = 0
        for i in range(L):
            for m in mats:
                out["blk.%d.%s.weight" % (i, m)] = cyc[k % len(cyc)]
                k += 1
    else:
        t = NAME_TO_GGML[mix]
        # the reference has no Q5_K branch in embed_tokens (it zero-fills, transformer.cpp:595-598),
        # so a plain-Q5_K test file keeps a Q4_K embedding like real llama.cpp K-quant files do
        out["token_embd.weight"] = GGML_Q4_K if t == GGML_Q5_K else t
        out["output.weight"] = t
        for i in range(L):
            for m in mats:
                out["blk.%d.%s.weight" % (i, m)] = t
    return out


def gpt2_byte_alphabet() -> List[bytes]:
    """The 256 single-'character' tokens of GPT-2 byte-level BPE (reference tokenizer.cpp:14-52)."""
    out, n = [], 0
    for b in range(256):
        ident = (33 <= b <= 126) or (161 <= b <= 172) or (174 <= b <= 255)
        cp = b if ident else 256 + n
        if not ident:
            n += 1
        out.append(chr(cp).encode("utf-8"))
    return out


def synth_vocab(shape: LlamaShape, rng: np.random.Generator) -> Tuple[List[bytes], List[int]]:
    """GPT2-BPE style vocab: 256 byte tokens (so 'Ġ' exists and GPT2 mode triggers, tokenizer.cpp:80-81),
    special BOS/EOS as control tokens, remaining ids = unique multi-byte merges of ASCII letters."""
    alpha = gpt2_byte_alphabet()
    toks: List[bytes] = list(alpha)
    types = [1] * 256
    letters = [alpha[c] for c in b"abcdefghijklmnopqrstuvwxyz"] + [alpha[0x20]]
    seen = set(toks)
    i = 0
    while len(toks) < shape.vocab:
        tid = len(toks)
        if tid in (shape.bos, shape.eos):
            toks.append(b"<|special_%d|>" % tid)
            types.append(3)
            continue
        ln = 2 + (i % 4)
        cand = b"".join(letters[int(k)] for k in rng.integers(0, len(letters), ln))
        i += 1
        if cand in seen:
            cand = cand + b"_%d" % tid
        seen.add(cand)
        toks.append(cand)
        types.append(1)
    return toks, types


def llama3_rope_factors(head_dim: int, theta: float, factor: float = 8.0, low_freq_factor: float = 1.0, high_freq_factor: float = 4.0,
                        orig_ctx: int = 8192) -> np.ndarray:
    """The Llama-3.1 frequency divisors a converter writes into rope_freqs.weight: float32 [head_dim / 2], computed in float64.  Pair i of wavelength
    2 pi theta^(2i/hd): 1 below orig_ctx / high, `factor` above orig_ctx / low, 1 / ((1 - s) / factor + s) with s = (orig_ctx / wavelen - low) / (high -
    low) in between."""
    i = np.arange(head_dim // 2, dtype=np.float64)
    wavelen = 2.0 * np.pi * np.power(np.float64(theta), 2.0 * i / head_dim)
    out = np.empty(head_dim // 2, np.float64)
    for j, w in enumerate(wavelen):
        if w < orig_ctx / high_freq_factor:
            out[j] = 1.0
        elif w > orig_ctx / low_freq_factor:
            out[j] = factor
        else:
            s = (orig_ctx / w - low_freq_factor) / (high_freq_factor - low_freq_factor)
            out[j] = 1.0 / ((1.0 - s) / factor + s)
    return out.astype(np.float32)


def make_synthetic_llama(path: str, shape: LlamaShape, mix: str = "Q8_0", seed: int = 20260925,
                         with_scores: bool = False, overrides: Optional[Dict[str, str]] = None,
                         rope_freqs: Optional[np.ndarray] = None, rope_scaling: Optional[Dict[str, object]] = None,
                         arch: str = "llama", qkv_bias=None, tied: bool = False, extra_tensors: Sequence[TensorSpec] = (),
                         qk_norm=None, extra_kvs: Sequence[bytes] = (), experts: Optional[int] = None, experts_used: Optional[int] = None,
                         expert_inter: Optional[int] = None, router_scale: float = 1.0, moe_layers: Optional[Sequence[int]] = None) -> Dict[str, int]:
    """Write a seeded synthetic Llama-architecture GGUF; returns {tensor name: ggml type}.
    arch: general.architecture and the prefix of the hyper-parameter keys ("llama", "qwen2").  qkv_bias: None (no bias tensors) or the scale of the
    seeded blk.N.attn_{q,k,v}.bias vectors (F32 [out], normal values times the scale, written behind attn_v.weight as llama.cpp's converter orders them);
    a dict {"q": s, "k": s, "v": s} writes only the named ones.  tied: no output.weight (the LM head is token_embd.weight).  extra_tensors: appended as
    given (the loader's refusals: a bias of another type or size, tensors of architectures the engine does not run).
    qk_norm: None (no norm tensors) or the amplitude s of the seeded blk.N.attn_q_norm.weight / attn_k_norm.weight vectors (F32 [head_dim], 1 + s u with u
    uniform in [-1, 1), written behind attn_v.weight and any bias); a dict {"q": s, "k": s} writes only the named ones (the loader's pair rule).  A shape
    with head_dim != 0 gets <arch>.attention.key_length = value_length = head_dim and projections of heads x head_dim rows.  extra_kvs: metadata entries
    (kv_u32(...) ...) appended as given.  Without qk_norm, extra_kvs and shape.head_dim the file is byte for byte what it always was.
    experts: None (dense layers) or E -- the layers named by moe_layers (None: all of them) carry, in place of ffn_gate / ffn_up / ffn_down, the router
    blk.N.ffn_gate_inp.weight (F32, dims (hidden, E), normal values times router_scale / sqrt(hidden): logits of about that scale) and the 3-D expert
    tensors ffn_gate_exps / ffn_up_exps (dims (hidden, I_e, E)) and ffn_down_exps ((I_e, hidden, E)), expert e the contiguous block of rows e I_e .. (e + 1) I_e
    (hidden for down), in the types the mix gives ffn_gate / ffn_up / ffn_down of that layer (overrides: {"ffn_down_exps": "Q6_K"}); the keys
    <arch>.expert_count = E, <arch>.expert_used_count = experts_used and -- only where expert_inter is given -- <arch>.expert_feed_forward_length =
    expert_inter (without it I_e = shape.inter, what Mixtral files under `llama` carry).  Without `experts` the file is byte for byte what it always was.
    overrides: per-matrix types on top of the mix, in every layer ({"ffn_up": "Q4_K"}).
    rope_freqs: the per-pair frequency divisors, appended as the tensor rope_freqs.weight (float32; a float16 array is written as F16, any length is
    written as given: the loader's refusals).  rope_scaling: {"type": "linear" | "yarn" | ..., "factor": F, "original_context_length": N,
    "scale_linear": F (the legacy key)} -> the llama.rope.scaling.* / llama.rope.scale_linear keys that are named.  Both None: nothing is appended."""
    types = tensor_types(shape, mix)
    moe_at = set(range(shape.layers) if moe_layers is None else moe_layers) if experts else set()
    for i in sorted(moe_at):          # an expert tensor takes the type the mix gives the dense matrix in its place
        for m in ("ffn_gate", "ffn_up", "ffn_down"):
            types["blk.%d.%s_exps.weight" % (i, m)] = types.pop("blk.%d.%s.weight" % (i, m))
    for m, t in (overrides or {}).items():
        for i in range(shape.layers):
            if m.endswith("_exps") and i not in moe_at:
                continue
            if not m.endswith("_exps") and m.startswith("ffn_") and i in moe_at:
                continue
            types["blk.%d.%s.weight" % (i, m)] = NAME_TO_GGML[t]
    e_inter = int(expert_inter) if expert_inter else shape.inter
    hd = shape.hd
    q_dim, kv_dim = shape.heads * hd, shape.kv_heads * hd
    dims = {"attn_q": (shape.hidden, q_dim), "attn_k": (shape.hidden, kv_dim), "attn_v": (shape.hidden, kv_dim),
            "attn_output": (q_dim, shape.hidden), "ffn_gate": (shape.hidden, shape.inter),
            "ffn_up": (shape.hidden, shape.inter), "ffn_down": (shape.inter, shape.hidden)}

    def rng_for(name: str) -> np.random.Generator:
        h = 1469598103934665603
        for c in name.encode():
            h = ((h ^ c) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
        return np.random.Generator(np.random.Philox(key=[seed & 0xFFFFFFFFFFFFFFFF, h]))

    def norm_w(name: str) -> bytes:
        r = rng_for(name)
        return (1.0 + 0.05 * r.uniform(-1, 1, shape.hidden)).astype("<f4").tobytes()

    specs: List[TensorSpec] = []

    def mat(name: str, in_f: int, out_f: int, sigma: float = 1.0):
        t = types[name]
        specs.append(TensorSpec(name, (in_f, out_f), t,
                                (lambda n=name, tt=t, o=out_f, i=in_f, s=sigma: synth_tensor(rng_for(n), tt, o, i, s))))

    mat("token_embd.weight", shape.hidden, shape.vocab, sigma=float(np.sqrt(shape.hidden)))  # rows RMS ~ 1
    for i in range(shape.layers):
        p = "blk.%d." % i
        specs.append(TensorSpec(p + "attn_norm.weight", (shape.hidden,), GGML_F32, norm_w(p + "attn_norm.weight")))
        for m in ("attn_q", "attn_k", "attn_v"):
            mat(p + m + ".weight", *dims[m])
        for m, key in (("attn_q", "q"), ("attn_k", "k"), ("attn_v", "v")):
            scale = qkv_bias.get(key) if isinstance(qkv_bias, dict) else qkv_bias
            if scale is not None:
                name = p + m + ".bias"
                specs.append(TensorSpec(name, (dims[m][1],), GGML_F32, (float(scale) * rng_for(name).standard_normal(dims[m][1])).astype("<f4").tobytes()))
        for m, key in (("attn_q_norm", "q"), ("attn_k_norm", "k")):
            amp = qk_norm.get(key) if isinstance(qk_norm, dict) else qk_norm
            if amp is not None:
                name = p + m + ".weight"
                specs.append(TensorSpec(name, (hd,), GGML_F32, (1.0 + float(amp) * rng_for(name).uniform(-1, 1, hd)).astype("<f4").tobytes()))
        mat(p + "attn_output.weight", *dims["attn_output"])
        specs.append(TensorSpec(p + "ffn_norm.weight", (shape.hidden,), GGML_F32, norm_w(p + "ffn_norm.weight")))
        if i in moe_at:
            name = p + "ffn_gate_inp.weight"
            specs.append(TensorSpec(name, (shape.hidden, experts), GGML_F32,
                                    (float(router_scale) / np.sqrt(shape.hidden) * rng_for(name).standard_normal(experts * shape.hidden)).astype("<f4").tobytes()))
            for m, (in_f, out_f) in (("ffn_gate_exps", (shape.hidden, e_inter)), ("ffn_up_exps", (shape.hidden, e_inter)), ("ffn_down_exps", (e_inter, shape.hidden))):
                name, t = p + m + ".weight", types[p + m + ".weight"]
                specs.append(TensorSpec(name, (in_f, out_f, experts), t,
                                        (lambda n=name, tt=t, o=out_f, ii=in_f: synth_tensor(rng_for(n), tt, o * experts, ii, 1.0))))
            continue
        for m in ("ffn_gate", "ffn_up", "ffn_down"):
            mat(p + m + ".weight", *dims[m])
    specs.append(TensorSpec("output_norm.weight", (shape.hidden,), GGML_F32, norm_w("output_norm.weight")))
    if not tied:
        mat("output.weight", shape.hidden, shape.vocab, sigma=2.0)
    specs.extend(extra_tensors)

    toks, ttypes = synth_vocab(shape, np.random.Generator(np.random.Philox(key=[seed, 7])))
    kvs = [
        kv_str("general.architecture", arch),
        kv_str("general.name", "synthetic-%s-%s" % (shape.name, mix)),
        kv_u32("general.alignment", 32),
        kv_u32(arch + ".vocab_size", shape.vocab),
        kv_u32(arch + ".embedding_length", shape.hidden),
        kv_u32(arch + ".feed_forward_length", shape.inter),
        kv_u32(arch + ".block_count", shape.layers),
        kv_u32(arch + ".attention.head_count", shape.heads),
        kv_u32(arch + ".attention.head_count_kv", shape.kv_heads),
    ] + ([kv_u32(arch + ".attention.key_length", shape.head_dim), kv_u32(arch + ".attention.value_length", shape.head_dim)] if shape.head_dim else []) + [
        kv_u32(arch + ".context_length", shape.ctx),
        kv_f32(arch + ".attention.layer_norm_rms_epsilon", shape.eps),
        kv_f32(arch + ".rope.freq_base", shape.theta),
        kv_arr_str("tokenizer.ggml.tokens", toks),
        kv_arr_i32("tokenizer.ggml.token_type", ttypes),
        kv_u32("tokenizer.ggml.bos_token_id", shape.bos),
        kv_u32("tokenizer.ggml.eos_token_id", shape.eos),
    ]
    if with_scores:
        sc = -np.arange(shape.vocab, dtype=np.float32)  # earlier id = better merge
        kvs.append(kv_arr_f32("tokenizer.ggml.scores", sc))
    if rope_scaling:
        if "type" in rope_scaling:
            kvs.append(kv_str(arch + ".rope.scaling.type", str(rope_scaling["type"])))
        if "factor" in rope_scaling:
            kvs.append(kv_f32(arch + ".rope.scaling.factor", float(rope_scaling["factor"])))
        if "original_context_length" in rope_scaling:
            kvs.append(kv_u32(arch + ".rope.scaling.original_context_length", int(rope_scaling["original_context_length"])))
        if "scale_linear" in rope_scaling:
            kvs.append(kv_f32(arch + ".rope.scale_linear", float(rope_scaling["scale_linear"])))
    if experts:
        kvs.append(kv_u32(arch + ".expert_count", int(experts)))
        kvs.append(kv_u32(arch + ".expert_used_count", int(experts_used if experts_used is not None else 2)))
        if expert_inter:
            kvs.append(kv_u32(arch + ".expert_feed_forward_length", int(expert_inter)))
    kvs.extend(extra_kvs)
    if rope_freqs is not None:
        rf = np.asarray(rope_freqs)
        f16 = rf.dtype == np.float16
        specs.append(TensorSpec("rope_freqs.weight", (int(rf.size),), GGML_F16 if f16 else GGML_F32, rf.astype("<f2" if f16 else "<f4").tobytes()))
    write_gguf(path, kvs, specs)
    return types


def write_vocab_gguf(path: str, tokens: Sequence[bytes], scores: Optional[Sequence[float]], types: Sequence[int],
                     bos: int, eos: int) -> None:
    """A GGUF that carries only a vocabulary (plus one dummy tensor): tokenizer fixtures."""
    kvs = [kv_str("general.architecture", "llama"), kv_str("general.name", "vocab-only"), kv_u32("general.alignment", 32),
           kv_u32("llama.embedding_length", 32), kv_u32("llama.attention.head_count", 1), kv_u32("llama.block_count", 0),
           kv_arr_str("tokenizer.ggml.tokens", tokens), kv_arr_i32("tokenizer.ggml.token_type", types),
           kv_u32("tokenizer.ggml.bos_token_id", bos), kv_u32("tokenizer.ggml.eos_token_id", eos)]
    if scores is not None:
        kvs.append(kv_arr_f32("tokenizer.ggml.scores", scores))
    write_gguf(path, kvs, [TensorSpec("dummy.weight", (32,), GGML_F32, np.zeros(32, "<f4").tobytes())])


def algorithmic_bytes_per_token(shape: LlamaShape, types: Dict[str, int], pos: int = 0) -> int:
    """B_tok of SURVEY.md section 8(d): matrices once in GGUF encoding + norms + KV r/w + 1 embedding row."""
    hd = shape.hd
    total = 0
    for name, t in types.items():
        if name == "token_embd.weight":
            total += row_bytes(t, shape.hidden)
            continue
        if name == "output.weight":
            total += row_bytes(t, shape.hidden) * shape.vocab
            continue
        m = name.split(".")[2]
        in_f, out_f = {"attn_q": (shape.hidden, shape.heads * hd), "attn_k": (shape.hidden, shape.kv_heads * hd),
                       "attn_v": (shape.hidden, shape.kv_heads * hd), "attn_output": (shape.heads * hd, shape.hidden),
                       "ffn_gate": (shape.hidden, shape.inter), "ffn_up": (shape.hidden, shape.inter),
                       "ffn_down": (shape.inter, shape.hidden)}[m]
        total += row_bytes(t, in_f) * out_f
    total += (2 * shape.layers + 1) * shape.hidden * 4
    total += 2 * shape.layers * shape.kv_heads * hd * 2 * (pos + 1)   # KV read, once per KV head
    total += 2 * shape.layers * shape.kv_heads * hd * 2               # KV write
    return total
