"""Q3_K (GGML type 11) on the Python side, no GPU: gguf.dequantize against a scalar per-column statement of ggml's block_q3_K
(hmask[32] | qs[64] | scales[12] | d; w = d (s - 32) (q - 4)), the row size, and the Q3_K_M tensor-type map."""
import numpy as np
import pytest

from ntransformer_amd import gguf as G


@pytest.mark.parametrize("case", ["random", "hmask_ones", "hmask_zeros", "scales_0_31_32_63"])
def test_dequantize_is_the_block_definition(case):
    rng = np.random.Generator(np.random.Philox(key=[20261126, 1]))
    blk = np.frombuffer(G.synth_tensor(rng, G.GGML_Q3_K, 4, 512), np.uint8).reshape(8, 110).copy()
    if case.startswith("hmask"): blk[:, 0:32] = 0xFF if case == "hmask_ones" else 0
    if case.startswith("scales"):   # s[k] = (0, 31, 32, 63)[k % 4]: low nibbles 0 F 0 F twice over, top bits 0 1 2 3 in every pair of byte 8 + k
        blk[:, 96:108] = [0x00, 0xFF, 0x00, 0xFF] * 2 + [0x00, 0x55, 0xAA, 0xFF]
    want = np.empty((8, 256), np.float64)
    for b, (hm, qs, a, d) in enumerate((x[0:32], x[32:96], [int(v) for v in x[96:108]], float(x[108:110].copy().view("<f2")[0])) for x in blk):
        s = [0] * 16
        for k in range(4):
            s[k], s[4 + k] = (a[k] & 15) | ((a[8 + k] >> 0) & 3) << 4, (a[4 + k] & 15) | ((a[8 + k] >> 2) & 3) << 4
            s[8 + k], s[12 + k] = (a[k] >> 4) | ((a[8 + k] >> 4) & 3) << 4, (a[4 + k] >> 4) | ((a[8 + k] >> 6) & 3) << 4
        for c in range(256):
            n, j, l = c >> 7, (c >> 5) & 3, c & 31
            q = ((int(qs[32 * n + l]) >> (2 * j)) & 3) | (((int(hm[l]) >> (4 * n + j)) & 1) << 2)
            want[b, c] = d * (s[8 * n + 2 * j + l // 16] - 32) * (q - 4)
    got = G.dequantize(blk.reshape(-1), G.GGML_Q3_K, 8 * 256).astype(np.float64)
    # (d, s - 32 and q - 4 are an FP16 value and small integers: both float32 products are exact, the float64 statement has the same value)
    assert np.array_equal(got, want.reshape(-1))
    if case.startswith("scales"): assert (got.reshape(8, 16, 16)[:, 2::4] == 0).all() and (got.reshape(8, 16, 16)[:, 0::4] != 0).any()


def test_row_bytes_type_tables_and_the_q3_k_m_map():
    Q3, Q4, Q5 = G.GGML_Q3_K, G.GGML_Q4_K, G.GGML_Q5_K
    assert G.BLOCK[Q3] == (256, 110) and G.row_bytes(Q3, 4096) == 16 * 110
    assert (Q3, G.DT_Q3_K, G.GGML_TO_DT[Q3], G.NAME_TO_GGML["Q3_K"], G.DT_Q2_K) == (11, 10, 10, 11, 7)
    shape = G.LlamaShape("l8", 256, 512, 8, 4, 2, 512)
    want = {"token_embd.weight": Q3, "output.weight": G.GGML_Q6_K}
    for i in range(8):   # L / 16 = 0: no Q5_K ffn_down; use_more_bits(i, 8) holds for i = 0, 3, 6, 7
        per = {"attn_q": Q3, "attn_k": Q3, "ffn_gate": Q3, "ffn_up": Q3, "attn_output": Q4, "attn_v": Q5 if i < 2 else Q4, "ffn_down": Q4 if i in (0, 3, 6, 7) else Q3}
        want.update({"blk.%d.%s.weight" % (i, m): v for m, v in per.items()})
    assert G.tensor_types(shape, "Q3_K_M") == want
    plain = G.tensor_types(shape, "Q3_K")
    assert plain.pop("output.weight") == G.GGML_Q6_K and set(plain.values()) == {Q3}
