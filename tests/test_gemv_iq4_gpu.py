"""GPU tests of IQ4_XS / IQ4_NL through the C ABI: the IQ4_XS decode repack (table indices in Q4_K's nibble chunk, an 8-byte row record of signed scales,
csrc/gemv_rp.hip) holds the GGUF weights bit for bit and unpacks to the GGUF bytes; the matrix-core GEMV over it, the raw-block GEMVs of both types, the
F32-MFMA prompt GEMM and the embedding gather compute W . x for W = gguf.dequantize(...), against the float64 product at the GEMV bar of
tests/test_gemv_q3_k_gpu.py, with that file's activations (an outlier channel, an all-zero super-block).
Run on the MI355X box:  python -m pytest tests/test_gemv_iq4_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from ntransformer_amd import _lib
from ntransformer_amd import gguf as G
from ntransformer_amd import ops
from ntransformer_amd.ops import DeviceBuffer as DB

pytestmark = pytest.mark.gpu
XS, NL, Q4, Q5, DT = G.GGML_IQ4_XS, G.GGML_IQ4_NL, G.GGML_Q4_K, G.GGML_Q5_K, G.GGML_TO_DT


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261126, seed]))


def tol_for(y, in_f):
    return 4e-6 * np.sqrt(in_f) * max(1.0, float(np.abs(y).max()))


def matrix(r, gt, out_f, in_f, rp=True):
    """(GGUF bytes, their repack on the device, the weights as float64 [out_f, in_f])"""
    raw = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    return raw, ops.rp_pack(DB.from_numpy(raw), out_f, in_f, DT[gt]) if rp else None, G.dequantize(raw, gt, out_f * in_f).astype(np.float64).reshape(out_f, in_f)


def activations(r, in_f, T=1):
    x = r.standard_normal((T, in_f)).astype(np.float32)
    x[:, 5] *= 300.0                       # an outlier channel
    if in_f >= 512: x[:, 256:512] = 0.0    # an all-zero super-block
    return x


@pytest.mark.parametrize("out_f,in_f", [(1, 256), (16, 512), (37, 1024), (130, 4096)])   # a single row, a partial tile, several super-blocks
def test_repack_holds_the_gguf_weights_and_unpacks_to_the_gguf_bytes(out_f, in_f):
    raw, rp, _ = matrix(rng(out_f + in_f), XS, out_f, in_f)
    tiles = (out_f + 15) // 16
    assert ops.rp_bytes(DT[XS], out_f, in_f) == tiles * (in_f // 256) * 2208 <= 1.04 * 16 * tiles * G.row_bytes(XS, in_f)   # 2 x 1024 B of indices + 160
    out = DB.from_numpy(np.full(out_f * in_f, np.nan, np.float32))
    _lib.check(_lib.lib().ntk_rp_dequant(out.ptr, rp.ptr, out_f, in_f, DT[XS], None), "rp_dequant")
    assert np.array_equal(out.numpy(np.float32).view(np.uint32), G.dequantize(raw, XS, out_f * in_f).view(np.uint32))
    assert np.array_equal(ops.rp_unpack(rp, out_f, in_f, DT[XS], raw.size).numpy(np.uint8)[:raw.size], raw)


# 130 x 2560: a ragged tile x 10 super-blocks; 4200 rows: two tiles per workgroup; 8192 columns: two column slices per row in the raw forms; "+4" / "+2": the
# matrix that many bytes into its buffer (136-byte blocks are 4-byte aligned, 18-byte blocks 2-byte); IQ4_NL: one block, 33 blocks (no multiple of 256 columns)
GEMV = [(f, XS, o, i, 0) for f in ("raw", "rp") for o, i in ((3, 256), (130, 2560), (4200, 512), (20, 8192))] + [("raw", XS, 37, 1024, 4)] + \
       [("raw", NL, 3, 32, 0), ("raw", NL, 37, 1056, 0), ("raw", NL, 20, 8192, 0), ("raw", NL, 37, 1056, 2)]


@pytest.mark.parametrize("form,gt,out_f,in_f,off", GEMV)
def test_gemv_matches_the_float64_product(form, gt, out_f, in_f, off):
    r = rng(7 * out_f + in_f)
    raw, rp, W = matrix(r, gt, out_f, in_f, rp=form == "rp")
    x = activations(r, in_f)[0]
    ref = W @ x.astype(np.float64)
    yd, xd = DB.from_numpy(np.full(out_f, np.nan, np.float32)), DB.from_numpy(x)
    buf = DB.from_numpy(np.concatenate([np.zeros(off, np.uint8), raw, np.zeros(32, np.uint8)]))
    if form == "rp": _lib.check(_lib.lib().ntk_gemv_rp(yd.ptr, rp.ptr, xd.ptr, out_f, in_f, DT[gt], None), "gemv_rp")
    else: _lib.check(_lib.lib().ntk_gemv(yd.ptr, buf.ptr + off, xd.ptr, out_f, in_f, DT[gt], None), "gemv")
    err = float(np.abs(yd.numpy(np.float32) - ref).max())
    print("%s %s+%d gemv %d x %d: max |dy| = %.3g (bar %.3g)" % (G.DT_NAME[DT[gt]], form, off, out_f, in_f, err, tol_for(ref, in_f)))
    assert err <= tol_for(ref, in_f)


# case: (formats of the segments, RMSNorm prologue, residual, SiLU pair); rows (130, 40, 40) x 2560 columns: a second wave, several workgroups per segment
FUSED = {"norm": ((XS,), True, False, False), "plain+resid": ((XS,), False, True, False), "norm+silu": ((XS, XS), True, False, True),
         "iq|iq|q5": ((XS, XS, Q5), True, False, False), "q5|iq": ((Q5, XS), False, False, False), "q4|iq": ((Q4, XS), True, False, False), "iq|q4": ((XS, Q4), False, False, False)}


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
    arr, d = (ops.GemvSeg * 2)(), DB.from_numpy(np.full(1 << 14, 7.0, np.float32))
    for i, gt in enumerate((XS, G.GGML_Q6_K)):
        arr[i].W, arr[i].y, arr[i].rows, arr[i].dtype = d.ptr, d.ptr, 16, int(DT[gt])
    assert _lib.lib().ntk_gemv_rp_fused(arr, 2, d.ptr, 256, None, 0.0, None, 0, None) == -1        # a pairing outside the launch table: NTK_E_DTYPE
    assert (d.numpy(np.float32) == 7.0).all()                                                      # ... and y untouched
    assert _lib.lib().ntk_gemv(d.ptr, d.ptr, d.ptr, 16, 256, G.DT_Q2_K, None) == -1                  # Q2_K stays out
    for gt in (XS, NL):                                                                             # three rows of an embedding: exact
        raw, toks = matrix(rng(3), gt, 40, 512, rp=False)[0], np.array([39, 0, 17], np.int32)
        out = DB.from_numpy(np.full(3 * 512, np.nan, np.float32))
        ops.embed_rows(out, DB.from_numpy(raw), DB.from_numpy(toks), 3, 512, DT[gt])
        assert np.array_equal(out.numpy(np.float32).view(np.uint32), G.dequantize(raw, gt, 40 * 512).reshape(40, 512)[toks].reshape(-1).view(np.uint32))


@pytest.mark.parametrize("gt", [XS, NL])
@pytest.mark.parametrize("T", [2, 17])   # the F32-MFMA prompt GEMM: less than one 16-token pass; two passes, the second ragged
def test_prompt_gemm_f32_mfma(T, gt, out_f=32, in_f=512):
    r = rng(T)
    raw, _, W = matrix(r, gt, out_f, in_f, rp=False)
    X = activations(r, in_f, T)
    ref = X.astype(np.float64) @ W.T
    Y = DB.from_numpy(np.full(T * out_f, np.nan, np.float32))
    ops.gemm_quant(Y, DB.from_numpy(raw), DB.from_numpy(X.reshape(-1)), T, out_f, in_f, DT[gt])
    assert np.abs(Y.numpy(np.float32).reshape(T, out_f) - ref).max() <= tol_for(ref, in_f)
