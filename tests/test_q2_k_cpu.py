"""Q2_K (GGML type 10) on the Python side, no GPU: gguf.dequantize against a scalar per-column statement of ggml's block_q2_K
(scales[16] | qs[64] | d | dmin; w = d (scales[s] & 15) q - dmin (scales[s] >> 4)), the row size, the type tables and the Q2_K_MIX tensor-type map."""
import numpy as np
import pytest

from ntransformer_amd import gguf as G

CASES = {"random": None, "scales_0": (0xF0, 0x00), "minima_0": (0x0F, 0x00), "nibbles_0F": (0x00, 0x0F), "nibbles_F0": (0x00, 0xF0), "nibbles_FF": (0x00, 0xFF),
         "qs_FF": None}   # (and-mask, or-mask) on the sixteen scale bytes


@pytest.mark.parametrize("case", sorted(CASES))
def test_dequantize_is_the_block_definition(case):
    rng = np.random.Generator(np.random.Philox(key=[20261127, 1]))
    blk = np.frombuffer(G.synth_tensor(rng, G.GGML_Q2_K, 4, 512), np.uint8).reshape(8, 84).copy()
    if CASES[case]: blk[:, 0:16] = (blk[:, 0:16] & CASES[case][0]) | CASES[case][1]
    if case == "qs_FF": blk[:, 16:80] = 0xFF
    want = np.empty((8, 256), np.float64)
    for b, x in enumerate(blk):
        d, dmin = (float(v) for v in x[80:84].copy().view("<f2"))
        for c in range(256):
            n, j, l = c >> 7, (c >> 5) & 3, c & 31
            q, s = (int(x[16 + 32 * n + l]) >> (2 * j)) & 3, int(x[8 * n + 2 * j + l // 16])
            want[b, c] = np.float32(d * (s & 15) * q) - np.float32(dmin * (s >> 4))   # (both products are exact; the difference is the one rounding)
    got = G.dequantize(blk.reshape(-1), G.GGML_Q2_K, 8 * 256)
    assert got.dtype == np.float32 and np.array_equal(got, want.astype(np.float32).reshape(-1))
    if case == "scales_0": assert (got <= 0).all() and (got < 0).any()
    if case == "minima_0": assert (got >= 0).all() and (got > 0).any()


def test_row_bytes_type_tables_and_the_q2_k_mix_map():
    Q2, Q3, Q4, Q6 = G.GGML_Q2_K, G.GGML_Q3_K, G.GGML_Q4_K, G.GGML_Q6_K
    assert G.BLOCK[Q2] == (256, 84) and G.row_bytes(Q2, 4096) == 16 * 84 and G.DT_NAME[G.DT_Q2_K] == "Q2_K"
    assert (Q2, G.DT_Q2_K, G.GGML_TO_DT[Q2], G.NAME_TO_GGML["Q2_K"]) == (10, 7, 7, 10)
    for kv_heads, v_t in ((2, Q4), (4, Q3)):   # 8 query heads: four per KV head, then two
        per = {"attn_q": Q2, "attn_k": Q2, "ffn_gate": Q2, "ffn_up": Q2, "attn_output": Q3, "ffn_down": Q3, "attn_v": v_t}
        want = {"token_embd.weight": Q2, "output.weight": Q6}
        want.update({"blk.%d.%s.weight" % (i, m): t for i in range(3) for m, t in per.items()})
        assert G.tensor_types(G.LlamaShape("l3", 256, 512, 3, 8, kv_heads, 512), "Q2_K_MIX") == want
    plain = G.tensor_types(G.LlamaShape("l3", 256, 512, 3, 8, 2, 512), "Q2_K")
    assert plain.pop("output.weight") == Q6 and set(plain.values()) == {Q2}
