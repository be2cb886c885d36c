"""GPU tests of Q2_K through the C ABI: the decode repack (the 2-bit plane and the scale | minimum bytes as they lie, csrc/gemv_rp.hip) holds the GGUF weights
bit for bit and unpacks to the GGUF bytes; the matrix-core GEMV over it, the raw-block GEMV (ntk_gemv_fused: ntk_gemv refuses the type), the F32-MFMA prompt
GEMM and the embedding gather compute W . x for W = gguf.dequantize(...), against the float64 product at the GEMV bar of tests/test_gemv_rp.py; x has an
outlier channel and an all-zero super-block.
Run on the MI355X box:  python -m pytest tests/test_gemv_q2_k_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from ntransformer_amd import _lib
from ntransformer_amd import gguf as G
from ntransformer_amd import ops
from ntransformer_amd.ops import DeviceBuffer as DB

pytestmark = pytest.mark.gpu
Q2, Q3, Q4, DT = G.GGML_Q2_K, G.GGML_Q3_K, G.GGML_Q4_K, G.GGML_TO_DT


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261127, seed]))


def tol_for(y, in_f):
    return 4e-6 * np.sqrt(in_f) * max(1.0, float(np.abs(y).max()))


def matrix(r, gt, out_f, in_f):
    """(GGUF bytes, their repack on the device, the weights as float64 [out_f, in_f])"""
    raw = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    return raw, ops.rp_pack(DB.from_numpy(raw), out_f, in_f, DT[gt]), G.dequantize(raw, gt, out_f * in_f).astype(np.float64).reshape(out_f, in_f)


def activations(r, in_f, T=1):
    x = r.standard_normal((T, in_f)).astype(np.float32)
    x[:, 5] *= 300.0                       # an outlier channel
    if in_f >= 512: x[:, 256:512] = 0.0    # an all-zero super-block
    return x


@pytest.mark.parametrize("out_f,in_f", [(1, 256), (16, 512), (37, 1024), (130, 4096)])   # a single row, a partial tile, several super-blocks
def test_repack_holds_the_gguf_weights_and_unpacks_to_the_gguf_bytes(out_f, in_f):
    raw, rp, _ = matrix(rng(out_f + in_f), Q2, out_f, in_f)
    tiles = (out_f + 15) // 16
    assert ops.rp_bytes(DT[Q2], out_f, in_f) == tiles * (in_f // 256) * 1344 <= 1.04 * 16 * tiles * G.row_bytes(Q2, in_f)   # 2 x 512 B of planes + 320
    out = DB.from_numpy(np.full(out_f * in_f, np.nan, np.float32))
    _lib.check(_lib.lib().ntk_rp_dequant(out.ptr, rp.ptr, out_f, in_f, DT[Q2], None), "rp_dequant")
    assert np.array_equal(out.numpy(np.float32).view(np.uint32), G.dequantize(raw, Q2, out_f * in_f).view(np.uint32))
    assert np.array_equal(ops.rp_unpack(rp, out_f, in_f, DT[Q2], raw.size).numpy(np.uint8)[:raw.size], raw)


# 130 x 2560: 9 workgroups of a ragged tile x 10 super-blocks, two items in the first waves; 4200 rows: two tiles per workgroup (the shared digit image
# behind a barrier); 8192 columns: two column slices per row in the raw form; "raw+4": the matrix 4 bytes into its buffer (84-byte blocks are 4-byte aligned)
@pytest.mark.parametrize("form,out_f,in_f", [(f, o, i) for f in ("raw", "rp", "raw+4") for o, i in ((3, 256), (130, 2560), (4200, 512), (20, 8192))])
def test_gemv_matches_the_float64_product(form, out_f, in_f):
    r = rng(7 * out_f + in_f)
    raw, rp, W = matrix(r, Q2, out_f, in_f)
    x = activations(r, in_f)[0]
    ref = W @ x.astype(np.float64)
    yd, xd = DB.from_numpy(np.full(out_f, np.nan, np.float32)), DB.from_numpy(x)
    off = 4 if form == "raw+4" else 0
    buf = DB.from_numpy(np.concatenate([np.zeros(off, np.uint8), raw, np.zeros(32, np.uint8)]))
    if form == "rp": _lib.check(_lib.lib().ntk_gemv_rp(yd.ptr, rp.ptr, xd.ptr, out_f, in_f, DT[Q2], None), "gemv_rp")
    else: ops.gemv_fused([(buf.ptr + off, yd, out_f, DT[Q2])], xd, in_f)
    err = float(np.abs(yd.numpy(np.float32) - ref).max())
    print("Q2_K %s gemv %d x %d: max |dy| = %.3g (bar %.3g)" % (form, out_f, in_f, err, tol_for(ref, in_f)))
    assert err <= tol_for(ref, in_f)


# case: (formats of the segments, RMSNorm prologue, residual, SiLU pair); rows (130, 40, 40) x 2560 columns: a second wave, several workgroups per segment
FUSED = {"norm": ((Q2,), True, False, False), "plain+resid": ((Q2,), False, True, False), "norm+silu": ((Q2, Q2), True, False, True),
         "q2|q2|q4": ((Q2, Q2, Q4), True, False, False), "q2|q2|q3": ((Q2, Q2, Q3), True, False, False), "q4|q2": ((Q4, Q2), False, False, False),
         "q3|q2": ((Q3, Q2), False, False, False)}


@pytest.mark.parametrize("case", sorted(FUSED))
def test_gemv_rp_fused_forms(case, in_f=2560):
    gts, norm, resid, silu = FUSED[case]
    rows = (130, 130) if silu else (130, 40, 40)[:len(gts)]
    r = rng(len(case))
    mats = [matrix(r, gt, o, in_f) for gt, o in zip(gts, rows)]
    x, nw, h = activations(r, in_f)[0], (1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32), r.standard_normal(rows[0]).astype(np.float32)
    x64 = x.astype(np.float64)
    xin = x64 / np.sqrt((x64 * x64).mean() + 1e-5) * nw if norm else x64
    refs = [m[2] @ xin for m in mats]
    ys = [DB.from_numpy(h.copy() if resid else np.full(o, np.nan, np.float32)) for o in rows]
    ops.gemv_rp_fused([(m[1], y, o, DT[gt]) for m, o, gt, y in zip(mats, rows, gts, ys)], DB.from_numpy(x), in_f, norm_w=DB.from_numpy(nw) if norm else None,
                      eps=1e-5, resid=ys[0] if resid else None, silu_pair=silu)
    if silu:   # d(silu(g) u) <= |silu'| |u| dg + |silu(g)| du with |silu'| <= 1.1, |silu(g)| <= |g|
        g, u = refs
        tol = 1.1 * tol_for(g, in_f) * float(np.abs(u).max()) + tol_for(u, in_f) * float(np.abs(g).max())
        assert np.abs(ys[0].numpy(np.float32) - g / (1.0 + np.exp(-g)) * u).max() <= tol
        return
    if resid: refs[0] = h.astype(np.float64) + refs[0]
    for y, ref in zip(ys, refs):
        assert np.abs(y.numpy(np.float32) - ref).max() <= tol_for(ref, in_f)


def test_refusals_and_embedding_gather():
    arr, d = (ops.GemvSeg * 2)(), DB.zeros(1 << 16)
    for i, gt in enumerate((Q2, G.GGML_Q6_K)):
        arr[i].W, arr[i].y, arr[i].rows, arr[i].dtype = d.ptr, d.ptr, 16, int(DT[gt])
    assert _lib.lib().ntk_gemv_rp_fused(arr, 2, d.ptr, 256, None, 0.0, None, 0, None) == -1        # a pairing outside the launch table: NTK_E_DTYPE
    assert ops.gemm_quant_ws(DB.zeros(4 * 2 * 16), d, DB.zeros(4 * 2 * 256), 2, 16, 256, DT[Q2]) == -1   # ntk_gemm_quant_f16: no FP16 decoder (the F32-MFMA form runs the prompt)
    raw, toks = matrix(rng(3), Q2, 40, 512)[0], np.array([39, 0, 17], np.int32)                     # three rows of a Q2_K embedding: exact
    out = DB.from_numpy(np.full(3 * 512, np.nan, np.float32))
    ops.embed_rows(out, DB.from_numpy(raw), DB.from_numpy(toks), 3, 512, DT[Q2])
    assert np.array_equal(out.numpy(np.float32).view(np.uint32), G.dequantize(raw, Q2, 40 * 512).reshape(40, 512)[toks].reshape(-1).view(np.uint32))


@pytest.mark.parametrize("T", [2, 17])   # the F32-MFMA prompt GEMM: less than one 16-token pass; two passes, the second ragged
def test_prompt_gemm_f32_mfma(T, out_f=32, in_f=512):
    r = rng(T)
    raw, _, W = matrix(r, Q2, out_f, in_f)
    X = activations(r, in_f, T)
    ref = X.astype(np.float64) @ W.T
    Y = DB.from_numpy(np.full(T * out_f, np.nan, np.float32))
    ops.gemm_quant(Y, DB.from_numpy(raw), DB.from_numpy(X.reshape(-1)), T, out_f, in_f, DT[Q2])
    assert np.abs(Y.numpy(np.float32).reshape(T, out_f) - ref).max() <= tol_for(ref, in_f)
