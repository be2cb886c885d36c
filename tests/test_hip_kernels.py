"""GPU parity tests for the operator surface: every ntk_* launcher against the oracle (the CPU restatement of
the reference kernel it replaces) on the same seeded inputs, through the C ABI.  Tolerances are stated per
test; integer/byte results (F16 cache contents from F32, embedding rows, argmax) must be bit-exact.

Run on the MI355X box:  python -m pytest tests -m gpu -x -q
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN
from kat_vectors import KATS
from ntransformer_amd import gguf as G
from ntransformer_amd import _lib, ops
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O

pytestmark = pytest.mark.gpu

QUANT = {"Q8_0": G.GGML_Q8_0, "Q4_0": G.GGML_Q4_0, "Q4_K": G.GGML_Q4_K, "Q5_K": G.GGML_Q5_K, "Q6_K": G.GGML_Q6_K}


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20260925, seed]))


def gemv_gpu(Wraw, x, out_f, in_f, dt, w_offset=0):
    """ntk_gemv with W placed `w_offset` bytes into its allocation (exercises the 2-byte-aligned path)."""
    Wd = DB(Wraw.nbytes + w_offset + 64)
    Wd.upload(Wraw, w_offset)
    xd = DB.from_numpy(x.astype(np.float32))
    yd = DB.from_numpy(np.full(out_f, np.nan, np.float32))   # poisoned output
    ops.launch_gemv(yd, Wd.at(w_offset), xd, out_f, in_f, dt)
    ops.synchronize()
    return yd.numpy(np.float32)


def tol_for(y, in_f):
    # F32 accumulation in a different association order than the oracle: error ~ eps * sqrt(in) * |terms|
    return 4e-6 * np.sqrt(in_f) * max(1.0, float(np.abs(y).max()))


# ------------------------------------------------------------------------------- reference KATs
@pytest.mark.parametrize("name", sorted(KATS))
def test_reference_kats_on_gpu(name):
    k = KATS[name]
    y = gemv_gpu(np.ascontiguousarray(k["W"]).view(np.uint8), k["x"], k["out"], k["in"], k["dtype"])
    assert np.allclose(y, k["expect"], atol=k["tol"], rtol=0), (name, y)


def test_reference_silu_rmsnorm_kats_on_gpu():
    g = DB.from_numpy(np.array([0.0, 1.0, -1.0, 2.0], np.float32))
    u = DB.from_numpy(np.ones(4, np.float32))
    ops.launch_silu_mul(g, g, u, 4)                      # in place, as reference ffn.cpp:127
    assert np.allclose(g.numpy(), [0.0, 0.731, -0.269, 1.762], atol=0.01)
    x = DB.from_numpy(np.array([1, 2, 3, 4], np.float32))
    w = DB.from_numpy(np.ones(4, np.float32))
    ops.launch_rmsnorm(x, x, w, 1, 4, 1e-5)              # in place, as reference transformer.cpp:659
    assert np.allclose(x.numpy(), np.array([1, 2, 3, 4]) / np.sqrt(7.5 + 1e-5), atol=1e-6)


# ------------------------------------------------------------------------------- GEMV vs oracle
SHAPES = [  # (out, in): tiny, partial slices, every Llama-3.1 8B / 70B (out,in) class (row-trimmed where huge)
    (3, 256), (64, 512), (257, 1024), (129, 2048), (512, 4096), (1024, 4096), (96, 8192), (515, 14336), (130, 28672),
]


@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("out_f,in_f", SHAPES)
def test_gemv_matches_oracle(qname, out_f, in_f):
    gt = QUANT[qname]
    r = rng(out_f * 7 + in_f + gt)
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    x = r.standard_normal(in_f).astype(np.float32)
    dt = G.GGML_TO_DT[gt]
    ref = O.gemv(W, x, out_f, in_f, dt)
    y = gemv_gpu(W, x, out_f, in_f, dt)
    assert np.isfinite(y).all()
    assert np.abs(y - ref).max() <= tol_for(ref, in_f), np.abs(y - ref).max()


@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("off", [2, 6, 14])
def test_gemv_unaligned_weights(qname, off):
    gt = QUANT[qname]
    out_f, in_f = 37, 1024
    r = rng(off + gt)
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    x = r.standard_normal(in_f).astype(np.float32)
    dt = G.GGML_TO_DT[gt]
    ref = O.gemv(W, x, out_f, in_f, dt)
    y = gemv_gpu(W, x, out_f, in_f, dt, w_offset=off)
    assert np.abs(y - ref).max() <= tol_for(ref, in_f)


# ------------------------------------------------------------------------------- batched prompt GEMM (MFMA) vs oracle
def gemm_gpu(Wraw, X, out_f, in_f, dt, w_offset=0, resid=None):
    T = X.shape[0]
    Wd = DB(Wraw.nbytes + w_offset + 64)
    Wd.upload(Wraw, w_offset)
    Xd = DB.from_numpy(np.ascontiguousarray(X, np.float32))
    Yd = DB.from_numpy(np.full((T, out_f), np.nan, np.float32) if resid is None else resid.astype(np.float32))
    ops.gemm_quant(Yd, Wd.at(w_offset), Xd, T, out_f, in_f, dt, resid=Yd if resid is not None else None)
    ops.synchronize()
    return Yd.numpy(np.float32).reshape(T, out_f)


@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("T,out_f,in_f", [(1, 3, 256), (2, 64, 512), (5, 257, 1024), (16, 512, 4096), (17, 129, 2048),
                                          (33, 96, 8192), (7, 40, 14336), (16, 130, 28672)])
def test_gemm_quant_matches_per_token_oracle(qname, T, out_f, in_f):
    """ntk_gemm_quant (one pass over W per 16 tokens, F32 MFMA) against the oracle's GEMV applied token by token --
    what the reference's prefill loop computes (attention.cpp:144-162, ffn.cpp:96-133)."""
    gt = QUANT[qname]
    r = rng(T * 1000 + out_f * 7 + in_f + gt)
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    X = r.standard_normal((T, in_f)).astype(np.float32)
    dt = G.GGML_TO_DT[gt]
    ref = np.stack([O.gemv(W, X[t], out_f, in_f, dt) for t in range(T)])
    Y = gemm_gpu(W, X, out_f, in_f, dt)
    assert np.isfinite(Y).all()
    assert np.abs(Y - ref).max() <= tol_for(ref, in_f), np.abs(Y - ref).max()


def gemm_ws_gpu(Wraw, X, out_f, in_f, dt, resid=None):
    T = X.shape[0]
    Wd = DB.from_numpy(Wraw)
    Xd = DB.from_numpy(np.ascontiguousarray(X, np.float32))
    Yd = DB.from_numpy(np.full((T, out_f), np.nan, np.float32) if resid is None else resid.astype(np.float32))
    st = ops.gemm_quant_ws(Yd, Wd, Xd, T, out_f, in_f, dt, resid=Yd if resid is not None else None)
    assert st == 0, st
    return Yd.numpy(np.float32).reshape(T, out_f)


@pytest.mark.parametrize("qname", ["Q8_0", "Q4_K", "Q6_K"])
@pytest.mark.parametrize("T,out_f,in_f", [(1, 16, 256), (5, 64, 512), (64, 128, 4096), (200, 48, 1024), (1100, 32, 256), (70, 32, 14336)])
def test_gemm_quant_f16_with_row_maxima_from_the_producers(qname, T, out_f, in_f):
    """The prompt GEMM's operand pre-pass without its own pass over X for the token scales: ntk_rmsnorm_rowmax and ntk_silu_mul_rowmax leave every
    token's largest |x| beside their output and ntk_gemm_quant_ws_rm takes it.  Against the separate launches (ntk_rmsnorm / ntk_silu_mul +
    ntk_gemm_quant_ws, which the tests around this one pin to the oracle): the producers' outputs, the maxima and the GEMM results are equal BIT FOR
    BIT -- rows of zeros, rows 1e15 / 1e20 times larger and 1100 tokens (two passes of 1024: the second takes row_max + 1024) included."""
    gt = QUANT[qname]
    dt = G.GGML_TO_DT[gt]
    r = rng(T * 31 + out_f + in_f + gt)
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    Wd = DB.from_numpy(W)
    h = r.standard_normal((T, in_f)).astype(np.float32)
    h[T // 2] = 0.0
    h[0] *= np.float32(1e15) if T > 1 else np.float32(1.0)
    nw = (1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32)
    eps = 1e-5
    # RMSNorm -> GEMM
    x1, x2 = DB.zeros(T * in_f * 4), DB.zeros(T * in_f * 4)
    rm, zz = DB.from_numpy(np.full(T, np.nan, np.float32)), DB.from_numpy(np.full(T, 7.0, np.float32))
    ops.launch_rmsnorm(x1, DB.from_numpy(h), DB.from_numpy(nw), T, in_f, eps)
    ops.launch_rmsnorm_rowmax(x2, DB.from_numpy(h), DB.from_numpy(nw), T, in_f, eps, rm, zz)
    X1 = x1.numpy(np.float32).reshape(T, in_f)
    assert np.array_equal(X1, x2.numpy(np.float32).reshape(T, in_f))
    assert np.array_equal(rm.numpy(np.float32), np.abs(X1).max(axis=1)) and not zz.numpy(np.float32).any()
    y1, y2 = DB.zeros(T * out_f * 4), DB.zeros(T * out_f * 4)
    assert ops.gemm_quant_ws(y1, Wd, x1, T, out_f, in_f, dt) == 0
    assert ops.gemm_quant_ws_rm(y2, Wd, x2, T, out_f, in_f, dt, rm) == 0
    Y1 = y1.numpy(np.float32)
    assert np.isfinite(Y1).all() and np.array_equal(Y1, y2.numpy(np.float32))
    # SiLU(gate) * up -> GEMM (+ residual epilogue)
    g = (2.0 * r.standard_normal((T, in_f))).astype(np.float32)
    u = r.standard_normal((T, in_f)).astype(np.float32)
    g[T // 2] = 0.0
    u[0] *= np.float32(1e20) if T > 1 else np.float32(1.0)
    a1, a2 = DB.zeros(T * in_f * 4), DB.from_numpy(g)
    ops.launch_silu_mul(a1, DB.from_numpy(g), DB.from_numpy(u), T * in_f)
    ops.launch_silu_mul_rowmax(a2, a2, DB.from_numpy(u), T, in_f, zz)            # in place over gate, maxima into the array the RMSNorm launch zeroed
    A1 = a1.numpy(np.float32).reshape(T, in_f)
    assert np.array_equal(A1, a2.numpy(np.float32).reshape(T, in_f))
    assert np.array_equal(zz.numpy(np.float32), np.abs(A1).max(axis=1))
    res = r.standard_normal((T, out_f)).astype(np.float32)
    y1, y2 = DB.from_numpy(res), DB.from_numpy(res)
    assert ops.gemm_quant_ws(y1, Wd, a1, T, out_f, in_f, dt, resid=y1) == 0
    assert ops.gemm_quant_ws_rm(y2, Wd, a2, T, out_f, in_f, dt, zz, resid=y2) == 0
    assert np.array_equal(y1.numpy(np.float32), y2.numpy(np.float32))


@pytest.mark.parametrize("qname", ["Q8_0", "Q4_K"])
@pytest.mark.parametrize("T,rows,in_f", [(64, 1024, 2048), (40, 512, 4096), (5, 64, 512), (200, 256, 1024), (1100, 64, 256)])
def test_gemm_quant_f16_split_sums_folded_into_the_consuming_launch(qname, T, rows, in_f):
    """A prompt projection's K splits summed by the launch that consumes it instead of a reduce launch (ntk_gemm_partials): Wo / down + residual +
    the next RMSNorm (ntk_gemm_quant_ws_deferred + ntk_reduce_rmsnorm_rowmax) and gate | up + SiLU x up (ntk_gemm_quant_ws_multi_deferred +
    ntk_reduce_silu_mul_rowmax), against the separate launches the tests around pin to the oracle: hidden, the normalised / activated rows and the
    token maxima equal BIT FOR BIT, whether the launch split K (nsplit > 1: the small-token shapes here) or not (nsplit = 1, and more than 1024
    tokens: each pass reduces itself)."""
    gt = QUANT[qname]
    dt = G.GGML_TO_DT[gt]
    r = rng(T * 13 + rows + in_f + gt)
    eps = 1e-5
    X = r.standard_normal((T, in_f)).astype(np.float32)
    Xd = DB.from_numpy(X)
    # (a) hidden += W . X, then RMSNorm of the new hidden
    W = DB.from_numpy(np.frombuffer(G.synth_tensor(r, gt, rows, in_f), np.uint8))
    h0 = r.standard_normal((T, rows)).astype(np.float32)
    nw = (1.0 + 0.1 * r.standard_normal(rows)).astype(np.float32)
    h1 = DB.from_numpy(h0)
    assert ops.gemm_quant_ws(h1, W, Xd, T, rows, in_f, dt, resid=h1) == 0
    x1 = DB.zeros(T * rows * 4)
    ops.launch_rmsnorm(x1, h1, DB.from_numpy(nw), T, rows, eps)
    h2, x2 = DB.from_numpy(h0), DB.zeros(T * rows * 4)
    rm, zz = DB.from_numpy(np.full(T, np.nan, np.float32)), DB.from_numpy(np.full(T, 3.0, np.float32))
    ns = ops.gemm_deferred_then_consumer("norm", W, Xd, T, rows, in_f, dt, hidden=h2, weight=DB.from_numpy(nw), eps=eps, x_out=x2, row_max_out=rm, zero=zz,
                                         in_place=(gt != G.GGML_Q4_K))   # (Q8_0: Y = resid = hidden, the engine's form; Q4_K: Y elsewhere, the consumer adds it)
    H1, X1 = h1.numpy(np.float32), x1.numpy(np.float32).reshape(T, rows)
    assert np.isfinite(H1).all() and np.array_equal(H1, h2.numpy(np.float32))
    assert np.array_equal(X1, x2.numpy(np.float32).reshape(T, rows))
    assert np.array_equal(rm.numpy(np.float32), np.abs(X1).max(axis=1)) and not zz.numpy(np.float32).any()
    # (b) silu(gate) * up of a two-matrix launch
    Wg = DB.from_numpy(np.frombuffer(G.synth_tensor(r, gt, rows, in_f), np.uint8))
    Wu = DB.from_numpy(np.frombuffer(G.synth_tensor(r, gt, rows, in_f), np.uint8))
    g1, u1 = DB.zeros(T * rows * 4), DB.zeros(T * rows * 4)
    assert ops.gemm_quant_ws_multi([(Wg, g1, rows, dt), (Wu, u1, rows, dt)], Xd, T, in_f) == 0
    a1 = DB.zeros(T * rows * 4)
    ops.launch_silu_mul(a1, g1, u1, T * rows)
    a2 = DB.zeros(T * rows * 4)
    ns2 = ops.gemm_deferred_then_consumer("silu", (Wg, Wu), Xd, T, rows, in_f, dt, output=a2, row_max_out=zz)
    A1 = a1.numpy(np.float32).reshape(T, rows)
    A2 = a2.numpy(np.float32).reshape(T, rows)
    assert np.isfinite(A1).all() and np.array_equal(A1, A2), (ns2, int((A1 != A2).sum()), float(np.abs(A1 - A2).max()), np.argwhere(A1 != A2)[:6].tolist())
    assert np.array_equal(zz.numpy(np.float32), np.abs(A1).max(axis=1))
    if (T, rows, in_f) == (64, 1024, 2048): assert ns > 1 and ns2 > 1   # (a narrow matrix at one chunk of tokens does split K)
    if T > 1024: assert ns == 1 and ns2 == 1


@pytest.mark.parametrize("qname", ["Q8_0", "Q4_K", "Q6_K"])
@pytest.mark.parametrize("T,rows,in_f", [(1, 16, 256), (5, 64, 512), (16, 256, 4096), (20, 128, 2048), (64, 1024, 2048), (70, 48, 1024), (200, 256, 1024), (1024, 32, 256)])
def test_gemm_quant_f16_planes_written_by_the_launch_that_produces_x(qname, T, rows, in_f):
    """The operand pre-pass inside the producers (ntk_gemm_prepare_x, ntk_rmsnorm_prepare_x, ntk_silu_mul_prepare_x, ntk_reduce_rmsnorm_prepare_x,
    ntk_reduce_silu_mul_prepare_x): the workgroup that writes a token's row splits it into the GEMM workspace and the projection runs with reuse_x = 1.
    Against the same chain with the GEMM's own pre-pass (pinned to the oracle by the tests around): the producers' outputs and every projection equal
    BIT FOR BIT -- rows of zeros and rows 1e15 times larger included, one chunk and several, K split or not."""
    gt = QUANT[qname]
    dt = G.GGML_TO_DT[gt]
    r = rng(T * 7 + rows + in_f + gt)
    eps = 1e-5
    W = DB.from_numpy(np.frombuffer(G.synth_tensor(r, gt, rows, in_f), np.uint8))
    h = r.standard_normal((T, in_f)).astype(np.float32)
    h[T // 2] = 0.0
    h[0] *= np.float32(1e15) if T > 1 else np.float32(1.0)
    nw = (1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32)
    ws = ops.gemm_workspace(in_f, rows)
    # (a) X as it lies
    y1, y2 = DB.zeros(T * rows * 4), DB.zeros(T * rows * 4)
    assert ops.gemm_quant_ws(y1, W, DB.from_numpy(h), T, rows, in_f, dt) == 0
    hd = DB.from_numpy(h)
    assert ops.prepare_x("x", ws, T, in_f, X=hd) == 0
    assert ops._gemm_quant_f16([(W, y2, rows, dt)], hd, T, in_f, workspace=ws, reuse_x=1) == 0
    Y1 = y1.numpy(np.float32)
    assert np.isfinite(Y1).all() and np.array_equal(Y1, y2.numpy(np.float32))
    # (b) RMSNorm -> projection (+ residual epilogue)
    x1, x2 = DB.zeros(T * in_f * 4), DB.zeros(T * in_f * 4)
    ops.launch_rmsnorm(x1, DB.from_numpy(h), DB.from_numpy(nw), T, in_f, eps)
    assert ops.prepare_x("rmsnorm", ws, T, in_f, output=x2, input=DB.from_numpy(h), weight=DB.from_numpy(nw), eps=eps) == 0
    assert np.array_equal(x1.numpy(np.float32), x2.numpy(np.float32))
    res = r.standard_normal((T, rows)).astype(np.float32)
    y1, y2 = DB.from_numpy(res), DB.from_numpy(res)
    assert ops.gemm_quant_ws(y1, W, x1, T, rows, in_f, dt, resid=y1) == 0
    assert ops._gemm_quant_f16([(W, y2, rows, dt)], x2, T, in_f, resid=y2, workspace=ws, reuse_x=1) == 0
    assert np.array_equal(y1.numpy(np.float32), y2.numpy(np.float32))
    # (c) SiLU(gate) * up -> projection, in place over gate
    g = (2.0 * r.standard_normal((T, in_f))).astype(np.float32)
    u = r.standard_normal((T, in_f)).astype(np.float32)
    g[T // 2] = 0.0
    u[0] *= np.float32(1e15) if T > 1 else np.float32(1.0)
    a1, a2 = DB.zeros(T * in_f * 4), DB.from_numpy(g)
    ops.launch_silu_mul(a1, DB.from_numpy(g), DB.from_numpy(u), T * in_f)
    assert ops.prepare_x("silu", ws, T, in_f, output=a2, gate=a2, up=DB.from_numpy(u)) == 0
    assert np.array_equal(a1.numpy(np.float32), a2.numpy(np.float32))
    y1, y2 = DB.zeros(T * rows * 4), DB.zeros(T * rows * 4)
    assert ops.gemm_quant_ws(y1, W, a1, T, rows, in_f, dt) == 0
    assert ops._gemm_quant_f16([(W, y2, rows, dt)], a2, T, in_f, workspace=ws, reuse_x=1) == 0
    assert np.array_equal(y1.numpy(np.float32), y2.numpy(np.float32))
    if in_f % 16 or rows % 32: return
    # (d) the consumers of deferred K splits: hidden += W . X, the next RMSNorm and ITS split in one launch; gate | up, SiLU x up and its split.  The
    # second projection (rows -> 16 rows) runs on the planes those launches wrote into the OTHER workspace.
    if rows % (128 if gt == G.GGML_Q8_0 else 256): return
    W2 = DB.from_numpy(np.frombuffer(G.synth_tensor(r, gt, 16, rows), np.uint8))
    ws2 = ops.gemm_workspace(rows, 16)
    Xd = DB.from_numpy(r.standard_normal((T, in_f)).astype(np.float32))
    h0 = r.standard_normal((T, rows)).astype(np.float32)
    nw2 = (1.0 + 0.1 * r.standard_normal(rows)).astype(np.float32)
    h1 = DB.from_numpy(h0)
    assert ops.gemm_quant_ws(h1, W, Xd, T, rows, in_f, dt, resid=h1) == 0
    x1 = DB.zeros(T * rows * 4)
    ops.launch_rmsnorm(x1, h1, DB.from_numpy(nw2), T, rows, eps)
    z1 = DB.zeros(T * 16 * 4)
    assert ops.gemm_quant_ws(z1, W2, x1, T, 16, rows, dt) == 0
    h2, x2, z2 = DB.from_numpy(h0), DB.zeros(T * rows * 4), DB.zeros(T * 16 * 4)
    pt, keep = _lib.GemmPartials(), []
    assert ops._gemm_quant_f16([(W, h2, rows, dt)], Xd, T, in_f, resid=h2, partials=pt, keep=keep) == 0
    assert ops.prepare_x("reduce_rmsnorm", ws2, T, rows, hidden=h2, partials=pt, weight=DB.from_numpy(nw2), eps=eps, x_out=x2) == 0
    assert ops._gemm_quant_f16([(W2, z2, 16, dt)], x2, T, rows, workspace=ws2, reuse_x=1) == 0
    assert np.array_equal(h1.numpy(np.float32), h2.numpy(np.float32)) and np.array_equal(x1.numpy(np.float32), x2.numpy(np.float32))
    assert np.array_equal(z1.numpy(np.float32), z2.numpy(np.float32))
    Wu = DB.from_numpy(np.frombuffer(G.synth_tensor(r, gt, rows, in_f), np.uint8))
    g1, u1, a1 = DB.zeros(T * rows * 4), DB.zeros(T * rows * 4), DB.zeros(T * rows * 4)
    assert ops.gemm_quant_ws_multi([(W, g1, rows, dt), (Wu, u1, rows, dt)], Xd, T, in_f) == 0
    ops.launch_silu_mul(a1, g1, u1, T * rows)
    assert ops.gemm_quant_ws(z1, W2, a1, T, 16, rows, dt) == 0
    g2, u2, a2 = DB.zeros(T * rows * 4), DB.zeros(T * rows * 4), DB.zeros(T * rows * 4)
    pt, keep = _lib.GemmPartials(), []
    assert ops._gemm_quant_f16([(W, g2, rows, dt), (Wu, u2, rows, dt)], Xd, T, in_f, partials=pt, keep=keep) == 0
    assert ops.prepare_x("reduce_silu", ws2, T, rows, output=a2, partials=pt) == 0
    assert ops._gemm_quant_f16([(W2, z2, 16, dt)], a2, T, rows, workspace=ws2, reuse_x=1) == 0
    assert np.array_equal(a1.numpy(np.float32), a2.numpy(np.float32)) and np.array_equal(z1.numpy(np.float32), z2.numpy(np.float32))


@pytest.mark.parametrize("T,nh,nkv,hd,interleaved,start_pos,max_seq", [(5, 4, 2, 64, 0, 0, 64), (70, 32, 8, 128, 0, 10, 128), (9, 6, 3, 80, 1, 3, 10), (64, 8, 8, 256, 0, 0, 64)])
def test_rope_kv_store_equals_rope_then_copy_to_kv_cache(T, nh, nkv, hd, interleaved, start_pos, max_seq):
    """ntk_rope_kv_store (a prompt's rotation and cache store as one launch) against ntk_rope + ntk_copy_to_kv_cache (reference attention.cpp:164-184,
    pinned to the oracle by test_rope / test_copy_to_kv_cache_is_bit_exact): the rotated q and both caches equal bit for bit, rows before start_pos and
    past the prompt untouched, rows that would fall past max_seq dropped (attention.cu:336)."""
    r = rng(T + nh + hd)
    q = r.standard_normal(T * nh * hd).astype(np.float32)
    k = r.standard_normal(T * nkv * hd).astype(np.float32)
    v = r.standard_normal(T * nkv * hd).astype(np.float32)
    pos = DB.from_numpy(np.arange(start_pos, start_pos + T, dtype=np.int32))
    junk = r.integers(0, 65536, max_seq * nkv * hd).astype(np.uint16)
    theta = 500000.0
    q1, k1 = DB.from_numpy(q), DB.from_numpy(k)
    kc1, vc1 = DB.from_numpy(junk), DB.from_numpy(junk[::-1].copy())
    ops.launch_rope(q1, k1, pos, 1, T, nh, nkv, hd, theta, 1.0, interleaved)
    ops.launch_copy_to_kv_cache(kc1, vc1, k1, DB.from_numpy(v), T, nkv, hd, start_pos, max_seq)
    q2, k2, v2 = DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v)
    kc2, vc2 = DB.from_numpy(junk), DB.from_numpy(junk[::-1].copy())
    ops.rope_kv_store(q2, k2, v2, pos, T, nh, nkv, hd, theta, 1.0, interleaved, kc2, vc2, start_pos, max_seq)
    assert np.array_equal(q1.numpy(np.float32), q2.numpy(np.float32))
    assert np.array_equal(k2.numpy(np.float32), k) and np.array_equal(v2.numpy(np.float32), v)          # k, v only read
    assert np.array_equal(kc1.numpy(np.uint16), kc2.numpy(np.uint16)) and np.array_equal(vc1.numpy(np.uint16), vc2.numpy(np.uint16))
    assert not np.array_equal(kc2.numpy(np.uint16), junk)


@pytest.mark.parametrize("qname", ["Q8_0", "Q4_0", "Q4_K", "Q5_K", "Q6_K"])
@pytest.mark.parametrize("T,out_f,in_f", [(1, 16, 256), (5, 64, 512), (64, 128, 4096), (37, 272, 1024), (100, 144, 2048), (9, 32, 768),
                                          (64, 1024, 4096), (130, 48, 8192), (20, 64, 14336), (64, 32, 28672), (300, 64, 512), (520, 48, 1024), (1100, 32, 256),
                                          (16, 14336, 4096), (12, 4096, 14336), (30, 2048, 4096)])
def test_gemm_quant_f16_matches_per_token_oracle(qname, T, out_f, in_f):
    """ntk_gemm_quant_ws (FP16 matrix cores, integer weights x two FP16 pieces of every scaled activation, 64 tokens per
    pass) against the oracle's GEMV applied token by token -- what the reference's prefill loop computes
    (attention.cpp:144-162, ffn.cpp:96-133): ragged token counts, 1 / 2 row tiles per wave, both row-tile geometries, the short-prompt
    form with the planes of a K slice in LDS (<= 32 tokens: one slice of 128 KB for the 14336 x 4096 matrix, 7 .. 28 slices for 14336 columns),
    K-quant sub-scales and minima, Q6_K's 16-column sub-scales, row pitches with and without dword alignment.  Same tolerance as
    the F32-MFMA path: the summation order differs and every activation carries at most one F32 ulp of rounding."""
    gt = QUANT[qname]
    r = rng(T * 1000 + out_f * 7 + in_f + gt + 1)
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    X = (r.standard_normal((T, in_f)) * np.exp(r.uniform(-6, 6, (T, 1)))).astype(np.float32)   # token scales over e^+-6: the per-token scale must absorb them
    dt = G.GGML_TO_DT[gt]
    ref = np.stack([O.gemv(W, X[t], out_f, in_f, dt) for t in range(T)])
    Y = gemm_ws_gpu(W, X, out_f, in_f, dt)
    assert np.isfinite(Y).all()
    for t in range(T):
        assert np.abs(Y[t] - ref[t]).max() <= tol_for(ref[t], in_f), (t, np.abs(Y[t] - ref[t]).max())
    R = r.standard_normal((T, out_f)).astype(np.float32)
    Y2 = gemm_ws_gpu(W, X, out_f, in_f, dt, resid=R)                                           # residual epilogue, in place
    assert np.array_equal(Y2, (R + Y).astype(np.float32)) or np.abs(Y2 - (R + Y)).max() <= 1e-6 * np.abs(Y).max()


@pytest.mark.parametrize("qname", ["Q8_0", "Q4_0", "Q4_K", "Q6_K"])
def test_gemm_quant_f16_short_prompts_give_the_same_bits_every_launch(qname):
    """The short-prompt form (K-slice-stationary, <= 32 tokens) three times over each of nine shapes -- slices of one unit and of many, one and two
    token blocks, one to 28 slices: identical bits every time.  (Found with exactly this check in round 6: an inline-asm conversion one wait state in
    front of the matrix instruction that reads it -- hipcc pads asm it cannot see into with one, the hardware wants two -- made whole tiles come out
    wrong differently from launch to launch in SOME builds, depending on what the scheduler happened to put between the two.)"""
    gt = QUANT[qname]
    dt = G.GGML_TO_DT[gt]
    for (T, rows, in_f) in [(5, 64, 512), (16, 128, 512), (16, 256, 4096), (3, 4096, 4096), (16, 2048, 4096), (9, 512, 14336), (20, 256, 4096),
                            (32, 1024, 2048), (17, 64, 8192)]:
        r = rng(T * 131 + rows + in_f + gt)
        Xd = DB.from_numpy((r.standard_normal((T, in_f)) * np.exp(r.uniform(-3, 3, (T, 1)))).astype(np.float32))
        W = DB.from_numpy(np.frombuffer(G.synth_tensor(r, gt, rows, in_f), np.uint8))
        ys = []
        for _ in range(3):
            y = DB.from_numpy(np.full((T, rows), np.nan, np.float32))
            assert ops.gemm_quant_ws(y, W, Xd, T, rows, in_f, dt) == 0
            ys.append(y.numpy(np.float32))
        assert np.isfinite(ys[0]).all() and np.array_equal(ys[0], ys[1]) and np.array_equal(ys[0], ys[2]), (T, rows, in_f)


@pytest.mark.parametrize("qname", ["Q4_K", "Q5_K", "Q6_K"])
@pytest.mark.parametrize("T,out_f,in_f", [(1, 16, 256), (5, 64, 512), (64, 128, 4096), (37, 272, 1024), (130, 48, 8192), (64, 32, 28672), (300, 64, 512),
                                          (200, 4096, 4096), (1100, 32, 256), (20, 4096, 14336)])
def test_gemm_quant_f16_reads_the_decode_repack_with_identical_bits(qname, T, out_f, in_f):
    """Round 6: with one resident copy of a K-quant matrix (the engine frees the uploaded GGUF bytes after the load-time repack) the prompt GEMM reads the
    REPACK itself (ntk_gemm_desc.weights_repacked; decoders DeqI<DT + GB_RP> of csrc/gemm_f16.hip over the tile-major layout of csrc/gemv_rp.hip) instead
    of an unpacked scratch copy: the same integers, the same scale products, the same operand slots and summation order as the raw-GGUF decoders -- so the
    results are IDENTICAL BITS, which pins the new decoders to everything the raw form is pinned to (the oracle's per-token GEMV, reference
    attention.cpp:144-162 / ffn.cpp:96-133).  One and two chunks per workgroup, K splits, ragged token counts, row tiles that are not whole 32-row
    pairs, the residual epilogue, two matrices in one launch."""
    gt = QUANT[qname]
    dt = G.GGML_TO_DT[gt]
    r = rng(T * 13 + out_f + in_f + gt)
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    X = (r.standard_normal((T, in_f)) * np.exp(r.uniform(-3, 3, (T, 1)))).astype(np.float32)
    Wd, Xd = DB.from_numpy(W), DB.from_numpy(X)
    Rp = ops.rp_pack(Wd, out_f, in_f, dt)
    y_raw = DB.from_numpy(np.full((T, out_f), np.nan, np.float32))
    y_rp = DB.from_numpy(np.full((T, out_f), np.nan, np.float32))
    assert ops.gemm_quant_ws(y_raw, Wd, Xd, T, out_f, in_f, dt) == 0
    assert ops.gemm_quant_ws(y_rp, Rp, Xd, T, out_f, in_f, dt, repacked=True) == 0
    a, b = y_raw.numpy(np.float32), y_rp.numpy(np.float32)
    assert np.isfinite(a).all() and np.array_equal(a, b), np.abs(a - b).max()
    if T <= 64:   # ... and against the oracle directly
        ref = np.stack([O.gemv(W, X[t], out_f, in_f, dt) for t in range(T)])
        bb = b.reshape(T, out_f)
        for t in range(T):
            assert np.abs(bb[t] - ref[t]).max() <= tol_for(ref[t], in_f)
    # residual epilogue, in place
    Rs = r.standard_normal((T, out_f)).astype(np.float32)
    y1, y2 = DB.from_numpy(Rs), DB.from_numpy(Rs)
    assert ops.gemm_quant_ws(y1, Wd, Xd, T, out_f, in_f, dt, resid=y1) == 0
    assert ops.gemm_quant_ws(y2, Rp, Xd, T, out_f, in_f, dt, resid=y2, repacked=True) == 0
    assert np.array_equal(y1.numpy(np.float32), y2.numpy(np.float32))
    # two matrices of the format in one launch (gate | up)
    if out_f >= 32:
        h = out_f // 2 // 16 * 16
        W2 = np.ascontiguousarray(W.reshape(out_f, -1)[:h]).reshape(-1)
        W2d = DB.from_numpy(W2)
        Rp2 = ops.rp_pack(W2d, h, in_f, dt)
        ya, yb = DB.from_numpy(np.zeros((T, out_f), np.float32)), DB.from_numpy(np.zeros((T, h), np.float32))
        yc, yd = DB.from_numpy(np.zeros((T, out_f), np.float32)), DB.from_numpy(np.zeros((T, h), np.float32))
        assert ops.gemm_quant_ws_multi([(Wd, ya, out_f, dt), (W2d, yb, h, dt)], Xd, T, in_f) == 0
        assert ops.gemm_quant_ws_multi([(Rp, yc, out_f, dt), (Rp2, yd, h, dt)], Xd, T, in_f, repacked=True) == 0
        assert np.array_equal(ya.numpy(np.float32), yc.numpy(np.float32)) and np.array_equal(yb.numpy(np.float32), yd.numpy(np.float32))
    assert ops.gemm_quant_ws(y_rp, Rp, Xd, T, out_f, in_f, G.GGML_TO_DT[G.GGML_Q8_0], repacked=True) == -1   # only the K-quant formats have a repack


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_gemm_quant_f16_random_sweep(seed):
    """tools/gemm_fuzz.py: 80 random (format, tokens, rows, columns, residual / several matrices) launches of the FP16 GEMM per seed
    against the oracle's per-token GEMV -- ragged chunks, odd chunk counts, ragged row tiles, both row-tile heights."""
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r_ = subprocess.run([sys.executable, os.path.join(root, "tools", "gemm_fuzz.py"), "--cases", "80", "--seed", str(seed)], capture_output=True,
                        text=True, timeout=600)
    assert r_.returncode == 0 and "gemm fuzz ok" in r_.stdout, (r_.stdout[-2000:], r_.stderr[-2000:])


@pytest.mark.parametrize("in_f", [128, 384, 640])
def test_gemm_quant_f16_q8_0_column_counts_of_half_a_sum_unit(in_f):
    """Q8_0 takes any multiple of 128 columns; the pre-pass lays the step sums out in units of 8 steps (256 columns) and writes a whole
    unit of zeros behind the last step -- with 128 columns left over that unit starts half a unit further: several chunks, so that an
    overrun of one chunk's area would land in the next chunk's planes."""
    gt = QUANT["Q8_0"]
    dt = G.GGML_TO_DT[gt]
    r = rng(in_f)
    T, out_f = 200, 48
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    X = r.standard_normal((T, in_f)).astype(np.float32)
    ref = np.stack([O.gemv(W, X[t], out_f, in_f, dt) for t in range(T)])
    Y = gemm_ws_gpu(W, X, out_f, in_f, dt)
    assert np.abs(Y - ref).max() <= tol_for(ref, in_f), np.abs(Y - ref).max()


@pytest.mark.parametrize("qname", ["Q8_0", "Q4_0", "Q4_K", "Q6_K"])
def test_gemm_quant_f16_outlier_channels_and_degenerate_tokens(qname):
    """The per-token scale of the FP16 split (csrc/gemm_f16.hip) under the activations that stress it: outlier channels 10^4 above the
    rest of the token (the small ones fall into the second piece's subnormal range: absolute error <= 2^-39 of the outlier), tokens
    of all zeros, tokens at the ends of the F32 range, one element per token.  Against the oracle's F32 GEMV; the bound is the
    split's: 2^-22 sum |w x| (both pieces' roundings, with room) plus the summation-order term of every other GEMM test."""
    gt = QUANT[qname]
    dt = G.GGML_TO_DT[gt]
    r = rng(4242 + gt)
    T, out_f, in_f = 70, 96, 2048
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    X = r.standard_normal((T, in_f)).astype(np.float32)
    X[0:20, ::97] *= 1e4                       # outlier channels
    X[20] = 0.0                                # a token of zeros
    X[21] = 0.0; X[21, 5] = 3.0                # one element
    X[22] *= 1e30; X[23] *= 1e-30              # ends of the F32 range (no overflow in s x: s = 2^(14 - exponent))
    X[24:30] *= np.exp(r.uniform(-20, 20, (6, in_f))).astype(np.float32)   # 17 orders of magnitude inside one token
    Wf = np.stack([O.embed_row(W, row, in_f, dt) for row in range(out_f)]).astype(np.float64)   # the dequantised weights (oracle's row decoder)
    ref = np.stack([O.gemv(W, X[t], out_f, in_f, dt) for t in range(T)])
    Y = gemm_ws_gpu(W, X, out_f, in_f, dt)
    assert np.isfinite(Y).all() and np.isfinite(ref).all()
    for t in range(T):
        bound = 2.0 ** -22 * (np.abs(Wf) @ np.abs(X[t].astype(np.float64))) + tol_for(ref[t], in_f)
        assert (np.abs(Y[t].astype(np.float64) - ref[t]) <= bound).all(), (t, np.abs(Y[t] - ref[t]).max(), bound.min())
    assert np.array_equal(Y[20], np.zeros(out_f, np.float32))


@pytest.mark.parametrize("qname", ["Q8_0", "Q4_0", "Q4_K", "Q6_K"])
@pytest.mark.parametrize("T,outs,in_f", [(20, (64, 32, 32), 512), (70, (4096, 1024, 1024), 4096), (300, (208, 208), 2048)])
def test_gemm_quant_f16_several_matrices_one_launch(qname, T, outs, in_f):
    """Q | K | V and gate | up as ONE launch of the FP16 GEMM (ntk_gemm_quant_ws_multi): every matrix against its own
    single-matrix launch, bit for bit (same tiles, same summation order), and against the oracle."""
    gt = QUANT[qname]
    dt = G.GGML_TO_DT[gt]
    r = rng(T + sum(outs) + in_f + gt)
    X = r.standard_normal((T, in_f)).astype(np.float32)
    Ws = [np.frombuffer(G.synth_tensor(r, gt, o, in_f), np.uint8) for o in outs]
    Xd = DB.from_numpy(X)
    Wd = [DB.from_numpy(w) for w in Ws]
    Yd = [DB.from_numpy(np.full((T, o), np.nan, np.float32)) for o in outs]
    st = ops.gemm_quant_ws_multi([(Wd[i], Yd[i], outs[i], dt) for i in range(len(outs))], Xd, T, in_f)
    assert st == 0, st
    for i, o in enumerate(outs):
        got = Yd[i].numpy(np.float32).reshape(T, o)
        alone = gemm_ws_gpu(Ws[i], X, o, in_f, dt)
        assert np.isfinite(got).all()
        for t in (0, T // 2, T - 1):
            ref = O.gemv(Ws[i], X[t], o, in_f, dt)
            assert np.abs(got[t] - ref).max() <= tol_for(ref, in_f)
        assert np.abs(got - alone).max() <= 1e-6 * max(1.0, np.abs(alone).max())   # (K split counts may differ between the two launches)
    other = G.DT_Q4_K if dt == G.DT_Q4_0 else G.DT_Q4_0
    assert ops.gemm_quant_ws_multi([(Wd[0], Yd[0], outs[0], dt), (Wd[1], Yd[1], outs[1], other)], Xd, T, in_f) == -2   # mixed formats


def test_gemm_quant_f16_full_size_and_rejections():
    """8B gate/up-sized matrix (14336 x 4096: the 2-row-tile geometry with 112 workgroups) and what the FP16 path refuses."""
    gt = G.GGML_Q8_0
    r = rng(99)
    out_f, in_f, T = 14336, 4096, 64
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    X = r.standard_normal((T, in_f)).astype(np.float32)
    Y = gemm_ws_gpu(W, X, out_f, in_f, G.GGML_TO_DT[gt])
    for t in (0, 31, 63):
        ref = O.gemv(W, X[t], out_f, in_f, G.GGML_TO_DT[gt])
        assert np.abs(Y[t] - ref).max() <= tol_for(ref, in_f)
    Wd, Xd, Yd = DB.zeros(1 << 16), DB.zeros(1 << 16), DB.zeros(1 << 16)
    assert ops.gemm_quant_ws(Yd, Wd, Xd, 2, 16, 256, G.DT_F16) == -1       # format outside the FP16 path: caller uses ntk_gemm_quant
    assert ops.gemm_quant_ws(Yd, Wd, Xd, 2, 10, 256, G.DT_Q8_0) == -2      # out_features not a multiple of 16
    assert ops.gemm_quant_ws(Yd, Wd, Xd, 2, 16, 320, G.DT_Q8_0) == -2      # in_features not whole units (Q8_0: 128 columns): the F32-MFMA path takes it
    assert ops.gemm_quant_ws(Yd, Wd, Xd, 2, 16, 288, G.DT_Q4_0) == -2


@pytest.mark.parametrize("qname", ["Q8_0", "Q4_0", "Q4_K", "Q5_K"])
def test_gemm_quant_f16_two_chunks_per_workgroup(qname):
    """A launch big enough for the 128-tokens-per-workgroup form (224 row tiles x 3 chunk pairs >= 512 workgroups): 300 tokens = 5
    chunks, so the last workgroup column has no second chunk (its planes are never written, its tokens never stored) and the last
    chunk is ragged.  Tokens of both halves of a pair, of the lone chunk and the last token against the oracle."""
    gt = QUANT[qname]
    dt = G.GGML_TO_DT[gt]
    r = rng(31 + gt)
    T, out_f, in_f = 300, 28672, 4096
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    X = (r.standard_normal((T, in_f)) * np.exp(r.uniform(-3, 3, (T, 1)))).astype(np.float32)
    R = r.standard_normal((T, out_f)).astype(np.float32)
    Y = gemm_ws_gpu(W, X, out_f, in_f, dt, resid=R)
    assert np.isfinite(Y).all()
    for t in (0, 63, 64, 127, 130, 200, 256, 299):
        ref = O.gemv(W, X[t], out_f, in_f, dt)
        assert np.abs(Y[t] - (R[t] + ref)).max() <= tol_for(ref, in_f), (t, np.abs(Y[t] - (R[t] + ref)).max())


@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("off", [2, 6, 14])
def test_gemm_quant_unaligned_weights_and_residual(qname, off):
    gt = QUANT[qname]
    T, out_f, in_f = 9, 37, 1024
    r = rng(off + gt + 77)
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    X = r.standard_normal((T, in_f)).astype(np.float32)
    R = r.standard_normal((T, out_f)).astype(np.float32)
    dt = G.GGML_TO_DT[gt]
    ref = np.stack([O.gemv(W, X[t], out_f, in_f, dt) for t in range(T)])
    assert np.abs(gemm_gpu(W, X, out_f, in_f, dt, w_offset=off) - ref).max() <= tol_for(ref, in_f)
    assert np.abs(gemm_gpu(W, X, out_f, in_f, dt, w_offset=off, resid=R) - (R + ref)).max() <= tol_for(ref, in_f)   # in place


def test_gemm_quant_equals_gemv_kernel_at_full_width():
    """Same weights, same activations: the MFMA prompt path and the decode GEMV agree to summation-order error at the
    8B shapes (16 tokens x 4096 -> 1024 rows of Q8_0 and Q4_K)."""
    for qname in ("Q8_0", "Q4_K", "Q6_K"):
        gt = QUANT[qname]
        T, out_f, in_f = 16, 1024, 4096
        r = rng(5 + gt)
        W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
        X = r.standard_normal((T, in_f)).astype(np.float32)
        dt = G.GGML_TO_DT[gt]
        Y = gemm_gpu(W, X, out_f, in_f, dt)
        for t in (0, 7, 15):
            y = gemv_gpu(W, X[t], out_f, in_f, dt)
            assert np.abs(Y[t] - y).max() <= tol_for(y, in_f)


def test_gemm_quant_rejects_bad_arguments():
    W, X, Y = DB.zeros(1 << 16), DB.zeros(1 << 16), DB.zeros(1 << 16)
    from ntransformer_amd import _lib
    L = _lib.lib()
    assert L.ntk_gemm_quant(Y.ptr, W.ptr, X.ptr, 2, 4, 100, G.DT_Q8_0, None, None) == -2       # in not a multiple of the block
    assert L.ntk_gemm_quant(Y.ptr, W.ptr, X.ptr, 2, 4, 256, 0, None, None) == -1                # dense F32: not a block format
    assert L.ntk_gemm_quant(Y.ptr, W.ptr + 1, X.ptr, 2, 4, 256, G.DT_Q4_K, None, None) == -4    # odd address
    assert L.ntk_gemm_quant(None, W.ptr, X.ptr, 2, 4, 256, G.DT_Q4_K, None, None) == -5
    assert L.ntk_gemm_quant(Y.ptr, W.ptr, X.ptr, 0, 4, 256, G.DT_Q4_K, None, None) == 0         # empty is fine


@pytest.mark.parametrize("gt,in_f", [(G.GGML_F32, 3), (G.GGML_F32, 1000), (G.GGML_F16, 1000), (G.GGML_F16, 4096), (G.GGML_F32, 4096)])
def test_gemv_dense(gt, in_f):
    out_f = 45
    r = rng(in_f + gt)
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    x = r.standard_normal(in_f).astype(np.float32)
    ref = O.gemv(W, x, out_f, in_f, G.GGML_TO_DT[gt])
    y = gemv_gpu(W, x, out_f, in_f, G.GGML_TO_DT[gt])
    assert np.abs(y - ref).max() <= tol_for(ref, in_f)


def test_gemv_add_f16():
    out_f, in_f = 300, 64          # the reference's delta "U . t" shape class
    r = rng(5)
    W = np.frombuffer(G.synth_tensor(r, G.GGML_F16, out_f, in_f), np.uint8)
    x = r.standard_normal(in_f).astype(np.float32)
    y0 = r.standard_normal(out_f).astype(np.float32)
    ref = O.gemv_add(y0, W, x, out_f, in_f, G.DT_F16)
    Wd, xd, yd = DB.from_numpy(W), DB.from_numpy(x), DB.from_numpy(y0)
    ops.launch_gemv_add(yd, Wd, xd, out_f, in_f, G.DT_F16)
    assert np.abs(yd.numpy() - ref).max() <= 1e-5
    with pytest.raises(Exception):
        ops.launch_gemv_add(yd, Wd, xd, out_f, in_f, G.DT_Q8_0)      # reference gemm.cu:866-868: F16 only


def test_gemv_rejects_bad_arguments():
    xd, yd = DB.zeros(4096 * 4), DB.zeros(64 * 4)
    Wd = DB.zeros(1 << 16)
    from ntransformer_amd import _lib
    L = _lib.lib()
    assert L.ntk_gemv(yd.ptr, Wd.ptr, xd.ptr, 4, 100, G.DT_Q8_0, None) == -2      # in not a multiple of the block
    assert L.ntk_gemv(yd.ptr, Wd.ptr, xd.ptr, 4, 128, 7, None) == -1               # Q2_K: unsupported (gemm.cu:801-803)
    assert L.ntk_gemv(None, Wd.ptr, xd.ptr, 4, 128, G.DT_Q8_0, None) == -5
    assert L.ntk_gemv(yd.ptr, Wd.ptr + 1, xd.ptr, 4, 256, G.DT_Q8_0, None) == -4   # odd address
    assert L.ntk_gemv(yd.ptr, Wd.ptr, xd.ptr, 0, 256, G.DT_Q8_0, None) == 0        # empty is fine


def test_gemv_full_size_linearity_and_lm_head():
    """Full 8B shapes: the LM head (128256 x 4096 Q8_0) against the oracle, and W(ax+by) = aWx + bWy on
    the 14336-wide down projection (size-independent property, no oracle involved)."""
    r = rng(11)
    out_f, in_f = 128256, 4096
    W = np.frombuffer(G.synth_tensor(r, G.GGML_Q8_0, out_f, in_f), np.uint8)
    x = r.standard_normal(in_f).astype(np.float32)
    y = gemv_gpu(W, x, out_f, in_f, G.DT_Q8_0)
    ref = O.gemv(W, x, out_f, in_f, G.DT_Q8_0)
    assert np.abs(y - ref).max() <= tol_for(ref, in_f)
    out_f, in_f = 4096, 14336
    W = np.frombuffer(G.synth_tensor(r, G.GGML_Q6_K, out_f, in_f), np.uint8)
    a, b = r.standard_normal(in_f).astype(np.float32), r.standard_normal(in_f).astype(np.float32)
    ya, yb = gemv_gpu(W, a, out_f, in_f, G.DT_Q6_K), gemv_gpu(W, b, out_f, in_f, G.DT_Q6_K)
    yc = gemv_gpu(W, (2 * a - 3 * b).astype(np.float32), out_f, in_f, G.DT_Q6_K)
    assert np.abs(yc - (2 * ya - 3 * yb)).max() <= 2e-4 * max(1.0, np.abs(yc).max())


# ------------------------------------------------------------------------------- fused GEMV
@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("in_f,rows", [(256, (64, 32, 32)), (4096, (512, 128, 128)), (8192, (256, 64, 64))])
def test_gemv_fused_norm_qkv(qname, in_f, rows):
    gt, dt = QUANT[qname], G.GGML_TO_DT[QUANT[qname]]
    r = rng(in_f + gt + 100)
    x = (r.standard_normal(in_f) * 3).astype(np.float32)
    nw = (1 + 0.05 * r.uniform(-1, 1, in_f)).astype(np.float32)
    Ws = [np.frombuffer(G.synth_tensor(r, gt, n, in_f), np.uint8) for n in rows]
    xn = O.rmsnorm(x, nw, 1e-5)
    refs = [O.gemv(W, xn, n, in_f, dt) for W, n in zip(Ws, rows)]
    xd, nd = DB.from_numpy(x), DB.from_numpy(nw)
    Wd = [DB.from_numpy(W) for W in Ws]
    yd = [DB.from_numpy(np.full(n, np.nan, np.float32)) for n in rows]
    ops.gemv_fused([(Wd[i], yd[i], rows[i], dt) for i in range(3)], xd, in_f, norm_w=nd, eps=1e-5)
    ops.synchronize()
    for i in range(3):
        assert np.abs(yd[i].numpy() - refs[i]).max() <= 2 * tol_for(refs[i], in_f)


@pytest.mark.parametrize("qname", ["Q4_K", "Q6_K"])
@pytest.mark.parametrize("outliers", [False, True])
@pytest.mark.parametrize("out_f,in_f,norm,resid,silu", [(64, 256, False, False, False), (300, 4096, True, False, False), (257, 4096, False, True, False),
                                                       (1024, 8192, True, False, True), (96, 2048, False, False, True), (40, 8192, False, True, False)])
def test_gemv_integer_activation_form(qname, out_f, in_f, norm, resid, silu, outliers):
    """The integer-activation form of the Q4_K / Q6_K GEMV (activations as three int8 digit planes per 32-column sub-block, products on
    v_dot4; gemv_core.hip.h XInt / DotI) -- normally taken only by launches of >= 48 MiB -- asked for by the call (ntk_debug_gemv_fused_form) and
    compared with the oracle at the GEMV's tolerance: plain, RMSNorm prologue, residual epilogue, gate|up + SiLU.  `outliers`: a few
    channels 1000 x the rest, the shape real Llama activations have and the synthetic ones lack (no checkpoint exists offline): the
    31 neighbours of an outlier in its sub-block keep up to 2^-22 of the OUTLIER as their error, which is what the form trades."""
    gt = QUANT[qname]
    dt = G.GGML_TO_DT[gt]
    r = rng(out_f + in_f + 3 * norm + 5 * resid + 7 * silu + gt)
    x = (r.standard_normal(in_f) * np.exp(r.uniform(-3, 3, in_f))).astype(np.float32)   # wide dynamic range inside every sub-block
    if outliers: x[r.choice(in_f, 4, replace=False)] *= 1000.0
    nw = (1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32)
    xin = O.rmsnorm(x[None, :], nw, 1e-5)[0] if norm else x
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    W2 = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    R = r.standard_normal(out_f).astype(np.float32)
    ref = O.gemv(W, xin, out_f, in_f, dt)
    if silu:
        up = O.gemv(W2, xin, out_f, in_f, dt)
        ref = (ref / (1.0 + np.exp(-ref.astype(np.float64))) * up).astype(np.float32)
    if resid: ref = ref + R
    xd, nwd = DB.from_numpy(x), DB.from_numpy(nw)
    yd = DB.from_numpy(R.copy() if resid else np.full(out_f, np.nan, np.float32))
    y2 = DB.zeros(out_f * 4)
    Wd, W2d = DB.from_numpy(W), DB.from_numpy(W2)
    segs = [(Wd, yd, out_f, dt)] + ([(W2d, y2, out_f, dt)] if silu else [])
    ops.gemv_fused(segs, xd, in_f, norm_w=nwd if norm else None, eps=1e-5, resid=yd if resid else None, silu_pair=silu,
                   integer_activations=True)   # (the form chosen by the call: ntk_debug_gemv_fused_form)
    got = yd.numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= tol_for(ref, in_f) * (4 if silu else 1), np.abs(got - ref).max()


@pytest.mark.parametrize("other", ["Q6_K", "Q5_K"])
@pytest.mark.parametrize("norm", [True, False])
@pytest.mark.parametrize("in_f,rows", [(256, (64, 32, 32)), (4096, (4096, 1024, 1024)), (8192, (8192, 1024, 1024))])
def test_gemv_fused_two_formats_one_launch(other, norm, in_f, rows):
    """llama.cpp's Q4_K_M stores attn_v as Q6_K (or Q5_K at 70B) beside Q4_K attn_q / attn_k: the fused norm + Q|K|V
    projection of such a layer is still ONE launch (workgroups split between the two decoders).  Same per-row arithmetic
    as the single-format launches, in both segment orders; checked against the oracle's rmsnorm + gemv."""
    gts = [G.GGML_Q4_K, G.GGML_Q4_K, QUANT[other]]
    r = rng(in_f + 977 + len(other))
    x = (r.standard_normal(in_f) * 3).astype(np.float32)
    nw = (1 + 0.05 * r.uniform(-1, 1, in_f)).astype(np.float32)
    Ws = [np.frombuffer(G.synth_tensor(r, gt, n, in_f), np.uint8) for gt, n in zip(gts, rows)]
    xn = O.rmsnorm(x, nw, 1e-5) if norm else x
    refs = [O.gemv(W, xn, n, in_f, G.GGML_TO_DT[gt]) for W, n, gt in zip(Ws, rows, gts)]
    xd, nd = DB.from_numpy(x), DB.from_numpy(nw)
    Wd = [DB.from_numpy(W) for W in Ws]
    for order in ([0, 1, 2], [2, 0, 1]):
        yd = [DB.from_numpy(np.full(n, np.nan, np.float32)) for n in rows]
        ops.gemv_fused([(Wd[i], yd[i], rows[i], G.GGML_TO_DT[gts[i]]) for i in order], xd, in_f, norm_w=nd if norm else None, eps=1e-5)
        ops.synchronize()
        for i in range(3):
            assert np.abs(yd[i].numpy() - refs[i]).max() <= 2 * tol_for(refs[i], in_f), (order, i)
    # three formats, or a residual / SiLU epilogue across formats, are refused (the engine then launches per format)
    with pytest.raises(Exception):
        ops.gemv_fused([(Wd[0], yd[0], rows[0], G.GGML_TO_DT[gts[0]]), (Wd[2], yd[2], rows[2], G.GGML_TO_DT[gts[2]])], xd, in_f, resid=yd[0])


@pytest.mark.parametrize("qname", ["Q8_0", "Q4_K", "Q6_K"])
@pytest.mark.parametrize("in_f,out_f", [(512, 256), (4096, 4096), (14336, 4096), (28672, 1024)])
def test_gemv_fused_residual_in_place(qname, in_f, out_f):
    gt, dt = QUANT[qname], G.GGML_TO_DT[QUANT[qname]]
    r = rng(in_f + out_f + gt)
    W = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    x = r.standard_normal(in_f).astype(np.float32)
    h = r.standard_normal(out_f).astype(np.float32)
    ref = h + O.gemv(W, x, out_f, in_f, dt)              # launch_gemv + launch_add_inplace
    Wd, xd, hd = DB.from_numpy(W), DB.from_numpy(x), DB.from_numpy(h)
    ops.gemv_fused([(Wd, hd, out_f, dt)], xd, in_f, resid=hd)
    ops.synchronize()
    assert np.abs(hd.numpy() - ref).max() <= tol_for(ref, in_f)


@pytest.mark.parametrize("qname", ["Q8_0", "Q4_K", "Q4_0", "Q6_K"])
@pytest.mark.parametrize("in_f,inter", [(256, 512), (4096, 1792), (8192, 515), (4096, 6144), (4096, 14336)])
def test_gemv_fused_norm_gate_up_silu(qname, in_f, inter):
    """(4096, 6144) and the real 8B shape (4096, 14336): half the waves of the launch get one gate / up pair more than the others;
    also through the integer-activation decoders."""
    gt, dt = QUANT[qname], G.GGML_TO_DT[QUANT[qname]]
    r = rng(in_f + inter + gt)
    x = r.standard_normal(in_f).astype(np.float32)
    nw = (1 + 0.05 * r.uniform(-1, 1, in_f)).astype(np.float32)
    Wg = np.frombuffer(G.synth_tensor(r, gt, inter, in_f), np.uint8)
    Wu = np.frombuffer(G.synth_tensor(r, gt, inter, in_f), np.uint8)
    xn = O.rmsnorm(x, nw, 1e-5)
    ref = O.silu_mul(O.gemv(Wg, xn, inter, in_f, dt), O.gemv(Wu, xn, inter, in_f, dt))
    xd, nd, gd, ud = DB.from_numpy(x), DB.from_numpy(nw), DB.from_numpy(Wg), DB.from_numpy(Wu)
    od, scratch = DB.from_numpy(np.full(inter, np.nan, np.float32)), DB.zeros(inter * 4)
    ops.gemv_fused([(gd, od, inter, dt), (ud, scratch, inter, dt)], xd, in_f, norm_w=nd, eps=1e-5, silu_pair=True)
    ops.synchronize()
    assert np.abs(od.numpy() - ref).max() <= 4 * tol_for(ref, in_f)
    if qname in ("Q4_K", "Q6_K") and inter >= 6144:   # ... and through the integer-activation decoders (every eligible launch)
        od2 = DB.from_numpy(np.full(inter, np.nan, np.float32))
        ops.gemv_fused([(gd, od2, inter, dt), (ud, scratch, inter, dt)], xd, in_f, norm_w=nd, eps=1e-5, silu_pair=True, integer_activations=True)
        ops.synchronize()
        assert np.abs(od2.numpy() - ref).max() <= 4 * tol_for(ref, in_f)


# ------------------------------------------------------------------------------- norm / rope / kv / attention
@pytest.mark.parametrize("batch,hidden", [(1, 256), (1, 4096), (3, 8192), (5, 1000)])
def test_rmsnorm(batch, hidden):
    r = rng(hidden)
    x = (r.standard_normal((batch, hidden)) * 2).astype(np.float32)
    w = (1 + 0.1 * r.standard_normal(hidden)).astype(np.float32)
    ref = O.rmsnorm(x, w, 1e-5)
    xd, wd, od = DB.from_numpy(x), DB.from_numpy(w), DB.zeros(x.nbytes)
    ops.launch_rmsnorm(od, xd, wd, batch, hidden, 1e-5)
    assert np.abs(od.numpy().reshape(batch, hidden) - ref).max() <= 2e-6 * np.abs(ref).max() + 1e-6
    hd_ = DB.zeros(x.size * 2)
    ops.launch_rmsnorm_f16(hd_, xd, wd, batch, hidden, 1e-5)
    got = hd_.numpy(np.float16).astype(np.float32).reshape(batch, hidden)
    assert np.abs(got - ref).max() <= 1e-3 * np.abs(ref).max()


@pytest.mark.parametrize("positions", [[0], [1], [4095], [3, 4, 5, 6, 100, 2047]])
@pytest.mark.parametrize("interleaved", [False, True])
def test_rope(positions, interleaved):
    nh, nkv, hd = 8, 2, 128
    T = len(positions)
    r = rng(T + 31 * interleaved + positions[0])
    q = r.standard_normal(T * nh * hd).astype(np.float32)
    k = r.standard_normal(T * nkv * hd).astype(np.float32)
    rq, rk = O.rope(q, k, positions, nh, nkv, hd, 500000.0, 1.0, interleaved)
    qd, kd, pd = DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(np.array(positions, np.int32))
    ops.launch_rope(qd, kd, pd, 1, T, nh, nkv, hd, 500000.0, 1.0, interleaved)
    # same F32 angle on both sides (the kernel rounds pow once, like libm); device sinf/cosf are within 2 ulp
    assert np.abs(qd.numpy() - rq).max() <= 1e-5
    assert np.abs(kd.numpy() - rk).max() <= 1e-5


@pytest.mark.parametrize("nh,nkv,hd", [(32, 8, 128), (8, 2, 64), (4, 4, 256)])
@pytest.mark.parametrize("interleaved", [False, True])
def test_rope_prompt_form_is_the_per_pair_kernel_bit_for_bit(nh, nkv, hd, interleaved):
    """From 4 tokens on ntk_rope evaluates a token's (cos, sin) pairs once for all heads (rope_rows_kernel); below it re-evaluates
    them per head and pair (rope_kernel, the 1:1 form).  Same frequency, same angle, same cosf / sinf: the prompt form, run token
    by token through the per-pair kernel (one-token launches), must give the same bits -- and both the oracle's values."""
    T = 37
    r = rng(nh + hd + 5 * interleaved)
    positions = [int(p_) for p_ in r.integers(0, 4096, T)]
    q = r.standard_normal(T * nh * hd).astype(np.float32)
    k = r.standard_normal(T * nkv * hd).astype(np.float32)
    qd, kd, pd = DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(np.array(positions, np.int32))
    ops.launch_rope(qd, kd, pd, 1, T, nh, nkv, hd, 500000.0, 1.0, interleaved)
    got_q, got_k = qd.numpy().copy(), kd.numpy().copy()
    one_q, one_k = np.empty_like(q), np.empty_like(k)
    for t in range(T):   # one-token launches: the per-pair kernel
        qt, kt = DB.from_numpy(q[t * nh * hd:(t + 1) * nh * hd]), DB.from_numpy(k[t * nkv * hd:(t + 1) * nkv * hd])
        ops.launch_rope(qt, kt, DB.from_numpy(np.array([positions[t]], np.int32)), 1, 1, nh, nkv, hd, 500000.0, 1.0, interleaved)
        one_q[t * nh * hd:(t + 1) * nh * hd] = qt.numpy(); one_k[t * nkv * hd:(t + 1) * nkv * hd] = kt.numpy()
    assert np.array_equal(got_q, one_q) and np.array_equal(got_k, one_k)
    rq, rk = O.rope(q, k, positions, nh, nkv, hd, 500000.0, 1.0, interleaved)
    assert np.abs(got_q - rq).max() <= 2e-5 and np.abs(got_k - rk).max() <= 2e-5


def test_copy_to_kv_cache_is_bit_exact():
    nkv, hd, max_seq, T, start = 2, 128, 16, 5, 9
    r = rng(77)
    k = (r.standard_normal(T * nkv * hd) * 10 ** r.uniform(-6, 4, T * nkv * hd)).astype(np.float32)
    v = r.standard_normal(T * nkv * hd).astype(np.float32)
    k[:4] = [65504.0, 65520.0, 1e-8, -0.0]
    kc, vc = np.zeros(max_seq * nkv * hd, np.uint16), np.zeros(max_seq * nkv * hd, np.uint16)
    O.copy_to_kv_cache(kc, vc, k, v, T, nkv, hd, start, max_seq)
    kcd, vcd = DB.zeros(kc.nbytes), DB.zeros(vc.nbytes)
    ops.launch_copy_to_kv_cache(kcd, vcd, DB.from_numpy(k), DB.from_numpy(v), T, nkv, hd, start, max_seq)
    assert np.array_equal(kcd.numpy(np.uint16), kc) and np.array_equal(vcd.numpy(np.uint16), vc)
    # positions past max_seq are dropped, not wrapped (reference attention.cu:336)
    ops.launch_copy_to_kv_cache(kcd, vcd, DB.from_numpy(k), DB.from_numpy(v), T, nkv, hd, max_seq - 2, max_seq)
    O.copy_to_kv_cache(kc, vc, k, v, T, nkv, hd, max_seq - 2, max_seq)
    assert np.array_equal(kcd.numpy(np.uint16), kc)


def make_cache(r, seq, max_seq, nkv, hd):
    kc = np.zeros(max_seq * nkv * hd, np.uint16)
    vc = np.zeros(max_seq * nkv * hd, np.uint16)
    kc[: seq * nkv * hd] = r.standard_normal(seq * nkv * hd).astype(np.float16).view(np.uint16)
    vc[: seq * nkv * hd] = r.standard_normal(seq * nkv * hd).astype(np.float16).view(np.uint16)
    return kc, vc


@pytest.mark.parametrize("seq", [1, 17, 140, 1025, 4096])
@pytest.mark.parametrize("nh,nkv,hd", [(32, 8, 128), (4, 2, 64), (6, 3, 80)])
def test_attention_decode(seq, nh, nkv, hd):
    if seq > 1025 and hd != 128:
        pytest.skip("long context only at the real head size")
    r = rng(seq + nh + hd)
    max_seq = max(seq, 32)
    kc, vc = make_cache(r, seq, max_seq, nkv, hd)
    q = r.standard_normal(nh * hd).astype(np.float32)
    scale = float(1 / np.sqrt(hd))
    ref = O.attention_decode(q, kc, vc, seq, nh, nkv, hd, max_seq, scale)
    od = DB.from_numpy(np.full(nh * hd, np.nan, np.float32))
    ops.launch_attention_decode(od, DB.from_numpy(q), DB.from_numpy(kc), DB.from_numpy(vc), seq, nh, nkv, hd, max_seq, scale)
    assert np.abs(od.numpy() - ref).max() <= 2e-5


@pytest.mark.parametrize("T,start", [(5, 0), (7, 3), (2, 130)])
def test_attention_prefill(T, start):
    nh, nkv, hd = 8, 2, 128
    r = rng(T + start)
    max_seq = 256
    kc, vc = make_cache(r, start + T, max_seq, nkv, hd)
    Q = r.standard_normal(T * nh * hd).astype(np.float32)
    scale = float(1 / np.sqrt(hd))
    ref = O.attention_prefill(Q, kc, vc, T, start, nh, nkv, hd, max_seq, scale)
    od = DB.from_numpy(np.full(T * nh * hd, np.nan, np.float32))
    ops.launch_attention_prefill(od, DB.from_numpy(Q), DB.from_numpy(kc), DB.from_numpy(vc), T, start, nh, nkv, hd, max_seq, scale)
    assert np.abs(od.numpy() - ref).max() <= 2e-5


@pytest.mark.parametrize("T,start,nh,nkv,hd", [(256, 0, 32, 8, 128), (256, 130, 32, 8, 128), (37, 5, 4, 2, 64), (33, 0, 8, 1, 128),
                                               (96, 1000, 64, 8, 128), (1, 7, 8, 2, 128), (70, 3, 4, 4, 256), (523, 41, 32, 8, 128)])
def test_attention_prefill_tiled_at_model_shapes(T, start, nh, nkv, hd):
    """The prompt attention kernels -- head_dim 128: the F16 matrix-core kernel (attention_mfma.hip: 64-query tiles, hi + lo
    F16 splits of q and p); other head sizes: the flash-style VALU kernel (32-query tiles; attention.hip) -- at the real
    head counts and prompt lengths where the 1:1 kernel's score rows and (nh, T) grid get large: against the oracle's
    restatement of the reference's attention_prefill_kernel (attention.cu:216-311), causal limit start_pos + query index,
    ragged last tile, GQA groups 1 / 2 / 4 / 8, and against the 1:1 launcher on the same inputs."""
    r = rng(T * 7 + start + nh)
    max_seq = max(512, start + T)
    kc, vc = make_cache(r, start + T, max_seq, nkv, hd)
    Q = r.standard_normal(T * nh * hd).astype(np.float32)
    scale = float(1 / np.sqrt(hd))
    ref = O.attention_prefill(Q, kc, vc, T, start, nh, nkv, hd, max_seq, scale)
    od = DB.from_numpy(np.full(T * nh * hd, np.nan, np.float32))
    ops.launch_attention_prefill(od, DB.from_numpy(Q), DB.from_numpy(kc), DB.from_numpy(vc), T, start, nh, nkv, hd, max_seq, scale)
    got = od.numpy()
    assert np.isfinite(got).all()
    assert np.abs(got - ref).max() <= 2e-5, np.abs(got - ref).max()


def test_attention_prefill_mfma_random_sweep():
    """40 random (tokens, start position, head counts) launches of the matrix-core prompt attention against the oracle: every
    combination of full / diagonal / ragged key tiles, waves with and without live queries, prefixes that end inside a tile (the
    clamped staging path of the launch's last tile), large score offsets (the rescale of the accumulators is skipped while no
    lane's maximum moves: it must not be skipped when one does)."""
    r = rng(4711)
    hd = 128
    for case in range(40):
        nkv = int(r.choice([1, 2, 8])); nh = nkv * int(r.choice([1, 2, 4]))
        T = int(r.choice([1, 2, 15, 16, 17, 63, 64, 65, 100, 128, 129, 200, 333]))
        start = int(r.choice([0, 0, 1, 7, 63, 64, 65, 100, 257]))
        max_seq = start + T + int(r.integers(0, 70))
        kc, vc = make_cache(r, start + T, max_seq, nkv, hd)
        Q = (r.standard_normal(T * nh * hd) * float(r.choice([0.1, 1.0, 6.0]))).astype(np.float32)   # x 6: maxima that keep moving
        scale = float(1 / np.sqrt(hd))
        ref = O.attention_prefill(Q, kc, vc, T, start, nh, nkv, hd, max_seq, scale)
        od = DB.from_numpy(np.full(T * nh * hd, np.nan, np.float32))
        ops.launch_attention_prefill(od, DB.from_numpy(Q), DB.from_numpy(kc), DB.from_numpy(vc), T, start, nh, nkv, hd, max_seq, scale)
        got = od.numpy()
        assert np.isfinite(got).all(), (case, T, start, nh, nkv)
        assert np.abs(got - ref).max() <= 2e-5 * max(1.0, float(np.abs(ref).max())), (case, T, start, nh, nkv, np.abs(got - ref).max())


@pytest.mark.parametrize("pos", [0, 1, 15, 16, 63, 300, 2047])
@pytest.mark.parametrize("nh,nkv,hd,table", [(32, 8, 128, True), (32, 8, 128, False), (4, 2, 64, True), (64, 8, 128, True), (6, 3, 80, False)])
def test_attention_decode_fused_equals_rope_store_attend(pos, nh, nkv, hd, table):
    r = rng(pos + nh)
    max_seq = 2048 if pos >= 512 else 512
    kc, vc = make_cache(r, pos, max_seq, nkv, hd)
    q = r.standard_normal(nh * hd).astype(np.float32)
    k = r.standard_normal(nkv * hd).astype(np.float32)
    v = r.standard_normal(nkv * hd).astype(np.float32)
    scale, theta = float(1 / np.sqrt(hd)), 500000.0
    # the reference's three launches (attention.cpp:165-190) on the oracle
    rq, rk = O.rope(q, k, [pos], nh, nkv, hd, theta)
    kc_ref, vc_ref = kc.copy(), vc.copy()
    O.copy_to_kv_cache(kc_ref, vc_ref, rk, v, 1, nkv, hd, pos, max_seq)
    ref = O.attention_decode(rq, kc_ref, vc_ref, pos + 1, nh, nkv, hd, max_seq, scale)
    kcd, vcd = DB.from_numpy(kc), DB.from_numpy(vc)
    od = DB.from_numpy(np.full(nh * hd, np.nan, np.float32))
    inv = None
    if table:   # the engine's host-computed table: 1/powf(theta, 2i/hd) in float32 (reference rotary.cu:47)
        i = np.arange(hd // 2, dtype=np.float32)
        inv = DB.from_numpy((np.float32(1.0) / np.power(np.float32(theta), (np.float32(2.0) * i) / np.float32(hd))).astype(np.float32))
    ops.attention_decode_fused(od, DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v), kcd, vcd,
                               DB.from_numpy(np.array([pos], np.int32)), nh, nkv, hd, max_seq, scale, theta, inv_freq=inv)
    assert np.abs(od.numpy() - ref).max() <= 3e-5
    # the stored row: V bit-exact; K within one half-precision ulp (device vs glibc sin/cos)
    assert np.array_equal(vcd.numpy(np.uint16), vc_ref)
    got_k = kcd.numpy(np.uint16).view(np.float16).astype(np.float32)
    want_k = kc_ref.view(np.float16).astype(np.float32)
    assert np.abs(got_k - want_k).max() <= 2e-3 * max(1.0, np.abs(want_k).max())
    assert np.array_equal(kcd.numpy(np.uint16)[: pos * nkv * hd], kc[: pos * nkv * hd])   # older rows untouched


@pytest.mark.parametrize("pos", [0, 1, 15, 31, 32, 33, 300, 543, 1023, 1024, 2047, 4095])
@pytest.mark.parametrize("nh,nkv,hd,nsplit", [(32, 8, 128, 8), (32, 8, 128, 32), (64, 8, 128, 32), (4, 2, 64, 3), (32, 8, 128, 1),
                                              (16, 1, 128, 17), (8, 8, 128, 16), (40, 8, 128, 19), (32, 8, 128, 16)])
def test_attention_decode_split_equals_oracle_and_single_pass(pos, nh, nkv, hd, nsplit):
    """Split-KV decode attention (long contexts): against the oracle's rope + store + attention and against the single-pass
    kernel; any number of splits, including more splits than positions.  head_dim 128 with 16 splits or more runs the matrix-core
    form (one workgroup per (KV head, split), attention_mfma.hip: 1 / 4 / 5 / 8 / 16 query heads per KV head, chunk boundaries at
    multiples of 32 positions), everything else the per-query-head walk."""
    r = rng(pos * 3 + nh + nsplit)
    max_seq = 4096 if pos >= 2048 else 2048
    kc, vc = make_cache(r, pos, max_seq, nkv, hd)
    q = r.standard_normal(nh * hd).astype(np.float32)
    k = r.standard_normal(nkv * hd).astype(np.float32)
    v = r.standard_normal(nkv * hd).astype(np.float32)
    scale, theta = float(1 / np.sqrt(hd)), 500000.0
    rq, rk = O.rope(q, k, [pos], nh, nkv, hd, theta)
    kc_ref, vc_ref = kc.copy(), vc.copy()
    O.copy_to_kv_cache(kc_ref, vc_ref, rk, v, 1, nkv, hd, pos, max_seq)
    ref = O.attention_decode(rq, kc_ref, vc_ref, pos + 1, nh, nkv, hd, max_seq, scale)
    outs, caches = [], []
    for split in (True, False):
        kcd, vcd = DB.from_numpy(kc), DB.from_numpy(vc)
        od = DB.from_numpy(np.full(nh * hd, np.nan, np.float32))
        args = (od, DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v), kcd, vcd, DB.from_numpy(np.array([pos], np.int32)),
                nh, nkv, hd, max_seq, scale, theta)
        if split: ops.attention_decode_split(*args, nsplit)
        else: ops.attention_decode_fused(*args)
        outs.append(od.numpy())
        caches.append((kcd.numpy(np.uint16), vcd.numpy(np.uint16)))
    assert np.isfinite(outs[0]).all()
    assert np.abs(outs[0] - ref).max() <= 3e-5
    assert np.abs(outs[0] - outs[1]).max() <= 2e-6                       # same math, different merge order (hd 128: q and p as two F16 pieces)
    assert np.array_equal(caches[0][0], caches[1][0]) and np.array_equal(caches[0][1], caches[1][1])   # identical cache rows


@pytest.mark.parametrize("pos,nsplit", [(8191, 32), (8191, 64), (32767, 32), (32767, 128), (131071, 32), (131071, 128)])
@pytest.mark.parametrize("nh,nkv", [(8, 2), (16, 2)])
def test_attention_decode_split_beyond_4096_positions(pos, nsplit, nh, nkv):
    """Contexts beyond 4096 (the reference takes -c / --ctx-size up to the file's 131072: main.cpp:74-75, transformer.cpp:70-73): the split
    attention at positions 8191 / 32767 / 131071 with the split count the engine uses there (Model::attention_splits: 32 at every context --
    measured best, profiles/r05_attention_long_context.txt) and a larger one, head_dim 128, both GQA ratios of the target models (4 and 8; two KV heads = a sample of the heads: the workgroups of
    a KV head share nothing with another's), against the ORACLE's rope + store + attention over the whole cache (reference attention.cu:108-202)."""
    hd, max_seq = 128, pos + 1
    r = rng(pos + nh + nsplit)
    kc, vc = make_cache(r, pos, max_seq, nkv, hd)
    q = r.standard_normal(nh * hd).astype(np.float32)
    k = r.standard_normal(nkv * hd).astype(np.float32)
    v = r.standard_normal(nkv * hd).astype(np.float32)
    scale, theta = float(1 / np.sqrt(hd)), 500000.0
    rq, rk = O.rope(q, k, [pos], nh, nkv, hd, theta)
    kc_ref, vc_ref = kc.copy(), vc.copy()
    O.copy_to_kv_cache(kc_ref, vc_ref, rk, v, 1, nkv, hd, pos, max_seq)
    ref = O.attention_decode(rq, kc_ref, vc_ref, pos + 1, nh, nkv, hd, max_seq, scale)
    kcd, vcd = DB.from_numpy(kc), DB.from_numpy(vc)
    od = DB.from_numpy(np.full(nh * hd, np.nan, np.float32))
    ops.attention_decode_split(od, DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v), kcd, vcd, DB.from_numpy(np.array([pos], np.int32)),
                               nh, nkv, hd, max_seq, scale, theta, nsplit)
    out = od.numpy()
    assert np.isfinite(out).all()
    assert np.abs(out - ref).max() <= 3e-5, np.abs(out - ref).max()
    row = slice(pos * nkv * hd, (pos + 1) * nkv * hd)
    got_k, got_v = kcd.numpy(np.uint16), vcd.numpy(np.uint16)
    assert np.array_equal(got_v[row], vc_ref[row])                                                  # V: bit-exact (RNE to half)
    dk = np.abs(got_k[row].view(np.float16).astype(np.float32) - kc_ref[row].view(np.float16).astype(np.float32))
    assert dk.max() <= 2e-3                                                                          # K: a half ulp at |k| < 4 (device vs glibc sin / cos at pos 131071)
    assert np.array_equal(got_k[: pos * nkv * hd], kc[: pos * nkv * hd]) and np.array_equal(got_v[: pos * nkv * hd], vc[: pos * nkv * hd])   # earlier rows untouched


@pytest.mark.parametrize("pos,nh,nkv,hd,nsplit", [
    (0, 32, 8, 128, 8), (3, 32, 8, 128, 8), (607, 32, 8, 128, 8), (1500, 32, 8, 128, 8), (1500, 32, 8, 128, 13), (2047, 32, 8, 64, 8), (900, 8, 8, 256, 8),
    (700, 12, 4, 64, 5), (3071, 32, 8, 128, 16), (4095, 32, 8, 128, 32), (4095, 64, 8, 128, 32), (2500, 40, 8, 128, 64), (1023, 16, 16, 128, 33),
    (5, 32, 8, 128, 32), (8191, 8, 2, 128, 32), (33000, 8, 2, 128, 32)])
def test_attention_decode_split_merged_equals_the_two_launch_form(pos, nh, nkv, hd, nsplit):
    """ntk_attention_decode_split_merged (one launch: the last workgroup of a head -- walk form -- or of a KV head -- matrix-core form -- merges the
    partial states, csrc/attention_merge.hip.h) against ntk_attention_decode_split (a second launch merges): the same operations in the same order, so
    the outputs are equal BIT FOR BIT, and so are the cache rows; three launches on one scratch (the arrival counters must return to zero).  The
    two-launch form is pinned to the oracle by the tests above and, at the shapes they do not hold -- (900, 8, 8, 256, 8), (700, 12, 4, 64, 5),
    (1023, 16, 16, 128, 33), (2500, 40, 8, 128, 64) --, by test_attention_head_sizes_gpu.py::test_attention_decode_split_at_the_merged_tests_shapes."""
    r = rng(pos * 5 + nh + nsplit)
    max_seq = max(2048, pos + 1)
    kc, vc = make_cache(r, pos, max_seq, nkv, hd)
    q = r.standard_normal(nh * hd).astype(np.float32)
    k = r.standard_normal(nkv * hd).astype(np.float32)
    v = r.standard_normal(nkv * hd).astype(np.float32)
    scale, theta = float(1 / np.sqrt(hd)), 500000.0
    outs = []
    for merged in (False, True):
        kcd, vcd = DB.from_numpy(kc), DB.from_numpy(vc)
        od = DB.from_numpy(np.full(nh * hd, np.nan, np.float32))
        args = (od, DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v), kcd, vcd, DB.from_numpy(np.array([pos], np.int32)),
                nh, nkv, hd, max_seq, scale, theta, nsplit)
        if merged: ops.attention_decode_split_merged(*args, launches=3)
        else: ops.attention_decode_split(*args)
        outs.append((od.numpy(), kcd.numpy(np.uint16), vcd.numpy(np.uint16)))
    assert np.isfinite(outs[0][0]).all()
    assert np.array_equal(outs[0][0], outs[1][0])
    assert np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])


def test_attention_decode_split_merged_refuses_more_than_64_splits():
    """One lane per split in the merging wave: 65 splits and more stay with the two-launch form (NTK_E_SHAPE, nothing launched)."""
    nh, nkv, hd, max_seq = 8, 2, 128, 2048
    z = lambda n: DB.zeros(n)
    with pytest.raises(Exception):
        ops.attention_decode_split_merged(z(nh * hd * 4), z(nh * hd * 4), z(nkv * hd * 4), z(nkv * hd * 4), z(max_seq * nkv * hd * 2), z(max_seq * nkv * hd * 2),
                                          DB.from_numpy(np.array([100], np.int32)), nh, nkv, hd, max_seq, 0.1, 500000.0, 65)


@pytest.mark.parametrize("pos", [5, 40, 607, 1500])
@pytest.mark.parametrize("nh,nkv,nsplit", [(32, 8, 8), (32, 8, 16), (64, 8, 32)])
def test_attention_decode_split_ignores_rows_past_the_position(pos, nh, nkv, nsplit):
    """Rows past the position (and the position's own row, which the launch writes itself) may hold anything -- NaN, infinities, the
    rows of an earlier sequence: the matrix-core form loads whole chunks of 32 rows before it knows the position and must mask by
    selects, never by arithmetic."""
    hd, max_seq = 128, 2048
    r = rng(pos * 7 + nh)
    kc, vc = make_cache(r, pos, max_seq, nkv, hd)
    junk = np.array([0x7E00, 0xFE00, 0x7C00, 0xFC00, 0x7BFF, 0xFBFF, 0x0001, 0x8000], np.uint16)   # NaN, -NaN, +-inf, +-65504, denormal, -0
    kc_j, vc_j = kc.copy(), vc.copy()
    kc_j[pos * nkv * hd:] = junk[r.integers(0, len(junk), kc.size - pos * nkv * hd)]
    vc_j[pos * nkv * hd:] = junk[r.integers(0, len(junk), vc.size - pos * nkv * hd)]
    q = r.standard_normal(nh * hd).astype(np.float32)
    k = r.standard_normal(nkv * hd).astype(np.float32)
    v = r.standard_normal(nkv * hd).astype(np.float32)
    scale, theta = float(1 / np.sqrt(hd)), 500000.0
    outs = []
    for kc0, vc0 in ((kc, vc), (kc_j, vc_j)):
        kcd, vcd = DB.from_numpy(kc0), DB.from_numpy(vc0)
        od = DB.from_numpy(np.full(nh * hd, np.nan, np.float32))
        ops.attention_decode_split(od, DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v), kcd, vcd,
                                   DB.from_numpy(np.array([pos], np.int32)), nh, nkv, hd, max_seq, scale, theta, nsplit)
        outs.append((od.numpy(), kcd.numpy(np.uint16), vcd.numpy(np.uint16)))
    assert np.isfinite(outs[0][0]).all()
    assert np.array_equal(outs[0][0], outs[1][0])                         # bit for bit: the junk took no part
    n_row = (pos + 1) * nkv * hd
    assert np.array_equal(outs[0][1][:n_row], outs[1][1][:n_row]) and np.array_equal(outs[0][2][:n_row], outs[1][2][:n_row])
    assert np.array_equal(outs[1][1][n_row:], kc_j[n_row:]) and np.array_equal(outs[1][2][n_row:], vc_j[n_row:])   # later rows untouched


# ------------------------------------------------------------------------------- small ops
def test_elementwise_and_reductions():
    r = rng(3)
    n = 10007
    a, b = r.standard_normal(n).astype(np.float32), r.standard_normal(n).astype(np.float32)
    ad, bd, od = DB.from_numpy(a), DB.from_numpy(b), DB.zeros(n * 4)
    ops.launch_add(od, ad, bd, n)
    assert np.array_equal(od.numpy(), a + b)
    ops.launch_add_inplace(ad, bd, n)
    assert np.array_equal(ad.numpy(), a + b)
    ops.launch_copy(od, bd, n)
    assert np.array_equal(od.numpy(), b)
    ops.launch_add_bias(od, bd, n)
    assert np.array_equal(od.numpy(), b + b)
    res = DB.zeros(4)
    ops.launch_cosine_similarity(res, DB.from_numpy(a), bd, n)
    assert abs(res.numpy()[0] - O.cosine_similarity(a, b)) <= 1e-6
    x = r.standard_normal((7, 333)).astype(np.float32)
    e = np.exp(x - x.max(1, keepdims=True))
    sd = DB.zeros(x.nbytes)
    ops.launch_softmax(sd, DB.from_numpy(x), 7, 333)
    assert np.abs(sd.numpy().reshape(7, 333) - e / e.sum(1, keepdims=True)).max() <= 1e-6
    mask = (r.uniform(size=(7, 333)) > 0.3).astype(np.uint8)
    mask[:, 0] = 1
    em = e * mask
    ops.launch_masked_softmax(sd, DB.from_numpy(x), DB.from_numpy(mask), 7, 333)
    xm = np.where(mask > 0, x, -np.inf)
    em = np.exp(xm - xm.max(1, keepdims=True))
    assert np.abs(sd.numpy().reshape(7, 333) - em / em.sum(1, keepdims=True)).max() <= 1e-6
    M, N, K = 9, 17, 33
    A, Bm = r.standard_normal((M, K)).astype(np.float32), r.standard_normal((N, K)).astype(np.float32)
    cd = DB.zeros(M * N * 4)
    ops.launch_gemm_f32(cd, DB.from_numpy(A), DB.from_numpy(Bm), M, N, K)
    assert np.abs(cd.numpy().reshape(M, N) - A @ Bm.T).max() <= 1e-4


@pytest.mark.parametrize("gt", [G.GGML_F32, G.GGML_F16, G.GGML_Q8_0, G.GGML_Q4_0, G.GGML_Q4_K, G.GGML_Q6_K])
def test_embed_rows_bit_exact(gt):
    vocab, hidden = 50, 512
    r = rng(gt + 1000)
    table = np.frombuffer(G.synth_tensor(r, gt, vocab, hidden, sigma=20.0), np.uint8)
    toks = np.array([0, 49, 7, 7, 23], np.int32)
    dt = G.GGML_TO_DT[gt]
    ref = np.stack([O.embed_row(table, int(t), hidden, dt) for t in toks])
    od = DB.from_numpy(np.full(toks.size * hidden, np.nan, np.float32))
    ops.embed_rows(od, DB.from_numpy(table), DB.from_numpy(toks), toks.size, hidden, dt)
    assert np.array_equal(od.numpy().reshape(toks.size, hidden), ref)


def test_embed_rows_q5_k_zero_fills_like_reference():
    vocab, hidden = 8, 256
    table = np.frombuffer(G.synth_tensor(rng(9), G.GGML_Q5_K, vocab, hidden), np.uint8)
    od = DB.from_numpy(np.full(hidden, np.nan, np.float32))
    st = ops.embed_rows(od, DB.from_numpy(table), DB.from_numpy(np.array([3], np.int32)), 1, hidden, G.DT_Q5_K, allow_unsupported=True)
    assert st == -1 and not od.numpy().any()


def test_argmax_first_maximum_and_advance_pos():
    r = rng(1)
    for n in (5, 512, 2048, 128256):
        x = r.standard_normal(n).astype(np.float32)
        a, b = sorted(r.choice(n, 2, replace=False))
        x[[a, b]] = x.max() + 1.0                      # exact tie: the lower index wins (sampler.cpp:18-28)
        tok, scratch = DB.zeros(64), DB.zeros(2 * 1024 * 4)
        ops.argmax(DB.from_numpy(x), n, tok, scratch)
        ops.synchronize()
        assert tok.numpy(np.int32)[0] == a == int(np.argmax(x))
    p = DB.from_numpy(np.array([41], np.int32))
    ops.advance_pos(p)
    ops.advance_pos(p)
    ops.synchronize()
    assert p.numpy(np.int32)[0] == 43


# ------------------------------------------------------------------------------- device sampler
@pytest.mark.parametrize("n,top_k,top_p,temp,pen", [(128256, 40, 0.9, 0.7, 1.1), (128256, 64, 0.5, 1.3, 1.0), (512, 8, 1.0, 0.2, 1.5),
                                                    (2049, 1, 0.9, 0.7, 1.1), (131072, 33, 0.95, 2.0, 1.2)])
def test_device_sampler_reproduces_the_host_sampler_stream(n, top_k, top_p, temp, pen):
    """ntk_sample_top_k (repeat penalty, temperature, top-k, softmax, top-p, cumulative walk on the device) against the
    engine's host sampler -- itself bit-identical to the reference's Sampler class on the golden draws
    (tests/test_host_logic.py) -- on the same logits, the same growing window of recent tokens and the same std::mt19937
    stream: the sampled token ids must be the same, draw for draw (reference src/inference/sampler.cpp:30-117)."""
    import ctypes as C
    from ntransformer_amd import engine as E
    L = E._bind()
    r = rng(n + top_k)
    logits = (r.standard_normal(n) * 3).astype(np.float32)
    logits[r.integers(0, n, 5)] += 6.0                     # a few dominant tokens so that repeats (and the penalty) occur
    n_draws, seed = 24, 1234
    p = E.GenParams(0, temp, top_k, top_p, pen, 16, seed, 0)
    recent0 = [int(t) for t in r.integers(0, n, 7)]
    want = (C.c_int * n_draws)()
    L.nt_sampler_draw.argtypes = [C.c_void_p, C.c_int, C.POINTER(E.GenParams), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]
    assert L.nt_sampler_draw(logits.ctypes.data_as(C.c_void_p), n, C.byref(p), (C.c_int * len(recent0))(*recent0), len(recent0), n_draws, want) == n_draws
    uni = np.zeros(n_draws, np.float32)
    L.nt_sampler_uniforms.argtypes = [C.c_uint64, C.c_int, C.c_void_p]
    assert L.nt_sampler_uniforms(seed, n_draws, uni.ctypes.data_as(C.c_void_p)) == n_draws
    recent, got = list(recent0), []
    d_out = DB.zeros(64)
    for d in range(n_draws):
        ld = DB.from_numpy(logits)                          # the penalty is applied in place: fresh logits per draw, like the host
        win = recent[-16:]                                  # repeat_window = 16
        rd = DB.from_numpy(np.asarray(win, np.int32))
        assert ops.sample_top_k(ld, n, rd, len(win), pen, temp, top_k, top_p, float(uni[d]), d_out) == 0
        got.append(int(d_out.numpy().view(np.int32)[0]))
        recent.append(got[-1])
    assert got == list(want), (got, list(want))
    assert len(set(got)) > 1 or top_k == 1
