"""IQ4_NL / IQ4_XS (GGML types 20 / 23) on the Python side and in both GGUF readers, no GPU: gguf.dequantize against the scalar block definitions
(IQ4_NL: d | qs[16], w = d k[idx]; IQ4_XS: d | scales_h | scales_l[4] | qs[128], w = d (ls - 32) k[idx]; k a fixed table of sixteen int8 values, a
sub-block's low nibbles its weights 0..15, the high ones 16..31), the row sizes, a written file through the numpy and the C++ reader, and the IQ4_XS map."""
import struct

import numpy as np
import pytest

from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G

NL, XS = G.GGML_IQ4_NL, G.GGML_IQ4_XS
K = [-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113]


@pytest.mark.parametrize("case", ["random", "all_sixteen_indices", "ls_0_31_32_63", "scales_h_ones"])
def test_dequantize_is_the_block_definition(case):
    rng = np.random.Generator(np.random.Philox(key=[20261126, 2]))
    xs = np.frombuffer(G.synth_tensor(rng, XS, 4, 512), np.uint8).reshape(8, 136).copy()
    nl = np.frombuffer(G.synth_tensor(rng, NL, 4, 64), np.uint8).reshape(8, 18).copy()
    if case == "all_sixteen_indices":   # byte j of a sub-block: index j below, 15 - j above
        xs[:, 8:136] = [j | ((15 - j) << 4) for j in range(16)] * 8
        nl[:, 2:18] = [j | ((15 - j) << 4) for j in range(16)]
    if case == "ls_0_31_32_63":         # ls[ib] = (0, 31, 32, 63)[ib % 4]: low nibbles 0 F 0 F, top bits 0 1 2 3
        xs[:, 2:8] = [0xE4, 0xE4, 0xF0, 0xF0, 0xF0, 0xF0]
    if case == "scales_h_ones": xs[:, 2:4] = 0xFF
    f32 = np.float32
    want = np.empty((8, 256), np.float32)
    for b, x in enumerate(xs):
        d, sh = x[0:2].copy().view("<f2").astype(f32)[0], int(x[2]) | int(x[3]) << 8
        for ib in range(8):
            ls = ((int(x[4 + ib // 2]) >> 4 * (ib & 1)) & 15) | (((sh >> 2 * ib) & 3) << 4)
            for j in range(16):
                q = int(x[8 + 16 * ib + j])
                want[b, 32 * ib + j], want[b, 32 * ib + 16 + j] = d * f32(ls - 32) * f32(K[q & 15]), d * f32(ls - 32) * f32(K[q >> 4])
    got = G.dequantize(xs.reshape(-1), XS, 8 * 256)
    assert np.array_equal(got.view(np.uint32), want.reshape(-1).view(np.uint32))
    if case == "ls_0_31_32_63": assert (got.reshape(8, 8, 32)[:, 2::4] == 0).all() and (got.reshape(8, 8, 32)[:, 0::4] != 0).all()
    want = np.empty((8, 32), np.float32)
    for b, x in enumerate(nl):
        d = x[0:2].copy().view("<f2").astype(f32)[0]
        for j in range(16):
            want[b, j], want[b, 16 + j] = d * f32(K[int(x[2 + j]) & 15]), d * f32(K[int(x[2 + j]) >> 4])
    assert np.array_equal(G.dequantize(nl.reshape(-1), NL, 8 * 32).view(np.uint32), want.reshape(-1).view(np.uint32))


def test_row_bytes_type_tables_and_the_iq4_xs_map():
    assert G.BLOCK[XS] == (256, 136) and G.row_bytes(XS, 4096) == 16 * 136 and G.BLOCK[NL] == (32, 18) and G.row_bytes(NL, 1056) == 33 * 18
    assert (NL, XS, G.DT_IQ4_NL, G.DT_IQ4_XS, G.GGML_TO_DT[NL], G.GGML_TO_DT[XS], G.NAME_TO_GGML["IQ4_XS"], G.DT_Q3_K) == (20, 23, 11, 12, 11, 12, 23, 10)
    assert [int(v) for v in G.IQ4_KVALUES] == K
    shape = G.LlamaShape("l16", 256, 512, 16, 4, 2, 512)
    want = {"token_embd.weight": XS, "output.weight": G.GGML_Q6_K}
    for i in range(16):   # L / 8 = 2: the first two ffn_down on Q5_K
        per = {m: XS for m in ("attn_q", "attn_k", "attn_output", "ffn_gate", "ffn_up")}
        per.update(attn_v=G.GGML_Q5_K, ffn_down=G.GGML_Q5_K if i < 2 else XS)
        want.update({"blk.%d.%s.weight" % (i, m): v for m, v in per.items()})
    assert G.tensor_types(shape, "IQ4_XS") == want
    assert set(G.tensor_types(shape, "IQ4_NL").values()) == {NL}


@pytest.mark.parametrize("mix", ["IQ4_XS", "IQ4_NL"])
def test_a_written_file_reads_back_through_both_readers_and_an_unknown_type_is_still_refused(mix, tmp_path):
    path, gt = str(tmp_path / (mix + ".gguf")), G.NAME_TO_GGML[mix]
    types = G.make_synthetic_llama(path, G.TINY, mix)
    f = G.read_gguf(path)
    by_name = {t["name"]: t for t in E.gguf_describe(path)["tensors"]}
    name = "blk.1.ffn_up.weight"
    ti, c = f.tensors[name], by_name[name]
    assert types[name] == ti.ggml_type == c["ggml_type"] == gt and c["type"] == mix and c["dtype"] == G.GGML_TO_DT[gt] == f.dtype(name)
    assert ti.nbytes == c["nbytes"] == 512 * G.row_bytes(gt, 256) and ti.offset == c["offset"]
    rms = lambda g: float(np.sqrt(np.mean(G.dequantize(np.array(g.raw(name)), gt, 512 * 256).astype(np.float64) ** 2)))
    assert 0.8 / 16 < rms(f) < 1.25 / 16   # the other formats' RMS, 1 / sqrt(in)
    f.close()
    # the C++ generator's file of the same mix: the same types by name, the same RMS
    synth = str(tmp_path / "synth.gguf")
    E.synth_write_gguf(synth, E.synth_spec("tiny", mix), 2)
    s = G.read_gguf(synth)
    assert {n: s.tensors[n].ggml_type for n in types} == types
    assert 0.8 / 16 < rms(s) < 1.25 / 16
    s.close()
    # type 20 and 23 became known; a neighbour did not (an early tensor: the C++ reader sizes an unknown type as F32, which has to fit the file)
    name = "blk.0.attn_k.weight"
    blob, key = bytearray(open(path, "rb").read()), name.encode()
    at = blob.index(struct.pack("<Q", len(key)) + key) + 8 + len(key)
    tpos = at + 4 + 8 * struct.unpack_from("<I", blob, at)[0]
    assert struct.unpack_from("<I", blob, tpos)[0] == gt
    struct.pack_into("<I", blob, tpos, 21)
    bad = str(tmp_path / "type21.gguf")
    open(bad, "wb").write(bytes(blob))
    with pytest.raises(KeyError):
        G.read_gguf(bad)
    assert {t["name"]: t["type"] for t in E.gguf_describe(bad)["tensors"]}[name] == "UNKNOWN"
