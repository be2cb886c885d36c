"""GPU tests of the prompt GEMMs (csrc/gemm_prefill.hip, csrc/gemm_f16.hip) and the embedding gather at Q8_0 / Q4_0 widths that are NOT multiples
of 256 columns.

  ntk_gemm_quant      (F32 MFMA, 16 tokens per pass) takes any multiple of 32 columns; gemm_quant_mfma_kernel<DT, false> is its ragged-tail
                      instantiation -- a last 256-column slice with fewer than eight 32-column sub-blocks (nsub < 8), a last K chunk shorter than the
                      others (clen) -- and is launched only when in % 256 != 0, which no other test does.
  ntk_gemm_quant_f16  (FP16 MFMA) takes Q8_0 at multiples of 128 columns (half a step-sum unit) and Q4_0 at multiples of 256; everything else it
                      must refuse without writing, because the engine then falls back to ntk_gemm_quant tensor by tensor.
  ntk_embed_rows      rows of 34 k / 18 k bytes: no row but the first starts 16-byte aligned.

The oracle is oracle.gemv applied token by token (oracle.embed_row for the gather); the bound is tol_for of tests/test_hip_kernels.py, as in
test_gemm_quant_matches_per_token_oracle / test_gemm_quant_f16_matches_per_token_oracle.  Every output buffer starts as NaN (or as the residual).

Run on the MI355X box:  python -m pytest tests/test_gemm_narrow_widths_gpu.py -m gpu -x -q
"""
import numpy as np
import pytest

from ntransformer_amd import gguf as G
from ntransformer_amd import ops
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O
from test_hip_kernels import gemm_gpu, gemm_ws_gpu, tol_for

pytestmark = pytest.mark.gpu

QUANT = {"Q8_0": G.GGML_Q8_0, "Q4_0": G.GGML_Q4_0}
NTK_E_SHAPE = -2


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(*key):
    return np.random.Generator(np.random.Philox(key=[20261021, sum(int(k) * 1000003 ** i for i, k in enumerate(key)) & 0xFFFFFFFFFFFFFFFF]))


def matrix(r, qname, rows, in_f):
    return np.frombuffer(G.synth_tensor(r, QUANT[qname], rows, in_f), np.uint8)


def per_token(W, X, out_f, in_f, dt):
    return np.stack([O.gemv(W, X[t], out_f, in_f, dt) for t in range(X.shape[0])])


# ------------------------------------------------------------------------------- (1) ntk_gemm_quant: the ragged-tail instantiation
@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("out_f", [3, 40, 129])
@pytest.mark.parametrize("T", [1, 5, 16, 17, 33])
@pytest.mark.parametrize("in_f", [32, 96, 320, 864, 2080, 2336, 4128])
def test_gemm_quant_ragged_tail_matches_per_token_oracle(qname, in_f, T, out_f):
    """32 / 96: one slice of 1 / 3 sub-blocks, seven of eight waves idle; 320 / 864: a second / fourth slice of 2 / 3 sub-blocks; 2080: a ninth slice of
    one sub-block alone in the second K chunk; 2336: two chunks, the second two slices long with one sub-block in its last; 4128: three chunks, the
    last one sub-block long.  1 .. 33 tokens: a partial pass, a full one, a full one + 1, two + 1; 3 / 40 / 129 rows: ragged row tiles."""
    dt = G.GGML_TO_DT[QUANT[qname]]
    r = rng(in_f, T, out_f, dt)
    W = matrix(r, qname, out_f, in_f)
    X = r.standard_normal((T, in_f)).astype(np.float32)
    ref = per_token(W, X, out_f, in_f, dt)
    Y = gemm_gpu(W, X, out_f, in_f, dt)
    assert np.isfinite(Y).all()
    err = float(np.abs(Y - ref).max())
    print("gemm_quant %s T=%d out=%d in=%d: max err %.3g, bound %.3g" % (qname, T, out_f, in_f, err, tol_for(ref, in_f)))
    assert err <= tol_for(ref, in_f), err


@pytest.mark.parametrize("qname", sorted(QUANT))
def test_gemm_quant_ragged_tail_residual_epilogue(qname):
    dt = G.GGML_TO_DT[QUANT[qname]]
    T, out_f, in_f = 17, 129, 864
    r = rng(dt, 1)
    W = matrix(r, qname, out_f, in_f)
    X = r.standard_normal((T, in_f)).astype(np.float32)
    R = r.standard_normal((T, out_f)).astype(np.float32)
    ref = per_token(W, X, out_f, in_f, dt)
    Y = gemm_gpu(W, X, out_f, in_f, dt, resid=R)                                     # in place
    assert np.isfinite(Y).all() and not np.array_equal(Y, R)
    err = float(np.abs(Y - (R + ref)).max())
    print("gemm_quant resid %s: max err %.3g, bound %.3g" % (qname, err, tol_for(ref, in_f)))
    assert err <= tol_for(ref, in_f), err


@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("off", [2, 6, 14])
def test_gemm_quant_ragged_tail_unaligned_weights(qname, off):
    """rows of 340 / 180 bytes starting 2 / 6 / 14 bytes into the allocation"""
    dt = G.GGML_TO_DT[QUANT[qname]]
    T, out_f, in_f = 5, 40, 320
    r = rng(off, dt, 2)
    W = matrix(r, qname, out_f, in_f)
    X = r.standard_normal((T, in_f)).astype(np.float32)
    ref = per_token(W, X, out_f, in_f, dt)
    Y = gemm_gpu(W, X, out_f, in_f, dt, w_offset=off)
    assert np.isfinite(Y).all()
    err = float(np.abs(Y - ref).max())
    print("gemm_quant %s w_off=%d: max err %.3g, bound %.3g" % (qname, off, err, tol_for(ref, in_f)))
    assert err <= tol_for(ref, in_f), err


# ------------------------------------------------------------------------------- (2) ntk_gemm_quant_f16: Q8_0 at half a sum unit
def scaled_tokens(r, T, in_f):
    return (r.standard_normal((T, in_f)) * np.exp(r.uniform(-6, 6, (T, 1)))).astype(np.float32)   # token scales over e^+-6


@pytest.mark.parametrize("T", [3, 20, 32, 33, 70])
@pytest.mark.parametrize("in_f", [128, 896, 2176, 4224])
def test_gemm_quant_f16_q8_0_at_odd_multiples_of_128_columns(in_f, T):
    """128-multiples that are not 256-multiples (896: a real hidden size), up to 32 tokens in the K-slice-stationary form and above it in the full one,
    per token within tol_for"""
    dt = G.DT_Q8_0
    out_f = 48
    r = rng(in_f, T, 3)
    W = matrix(r, "Q8_0", out_f, in_f)
    X = scaled_tokens(r, T, in_f)
    ref = per_token(W, X, out_f, in_f, dt)
    Y = gemm_ws_gpu(W, X, out_f, in_f, dt)
    assert np.isfinite(Y).all()
    worst = 0.0
    for t in range(T):
        e, b = float(np.abs(Y[t] - ref[t]).max()), tol_for(ref[t], in_f)
        worst = max(worst, e / b)
        assert e <= b, (t, e, b)
    print("gemm_f16 Q8_0 T=%d in=%d: worst err / bound %.3g" % (T, in_f, worst))


def test_gemm_quant_f16_q8_0_two_matrices_one_launch_at_896_columns():
    dt = G.DT_Q8_0
    T, in_f, outs = 20, 896, (64, 32)
    r = rng(4)
    Ws = [matrix(r, "Q8_0", o, in_f) for o in outs]
    X = scaled_tokens(r, T, in_f)
    Xd = DB.from_numpy(X)
    Wd = [DB.from_numpy(w) for w in Ws]
    Yd = [DB.from_numpy(np.full((T, o), np.nan, np.float32)) for o in outs]
    assert ops.gemm_quant_ws_multi([(Wd[i], Yd[i], outs[i], dt) for i in range(2)], Xd, T, in_f) == 0
    for i, o in enumerate(outs):
        got = Yd[i].numpy(np.float32).reshape(T, o)
        ref = per_token(Ws[i], X, o, in_f, dt)
        assert np.isfinite(got).all()
        for t in range(T):
            assert np.abs(got[t] - ref[t]).max() <= tol_for(ref[t], in_f), (i, t)


# ------------------------------------------------------------------------------- (3) refusals the engine's fallback relies on
@pytest.mark.parametrize("qname,in_f", [("Q8_0", 320), ("Q8_0", 864), ("Q4_0", 128), ("Q4_0", 384), ("Q4_0", 864)])
@pytest.mark.parametrize("T", [5, 40])
def test_gemm_quant_f16_refuses_other_widths_and_writes_nothing(qname, in_f, T):
    """not taken (NTK_E_SHAPE), every byte of the NaN output as it was: the engine then runs ntk_gemm_quant on that tensor (model_prompt.cpp)"""
    dt = G.GGML_TO_DT[QUANT[qname]]
    out_f = 32
    r = rng(in_f, T, dt, 5)
    Wd = DB.from_numpy(matrix(r, qname, out_f, in_f))
    Xd = DB.from_numpy(r.standard_normal((T, in_f)).astype(np.float32))
    before = np.full(T * out_f, np.nan, np.float32)
    Yd = DB.from_numpy(before)
    assert ops.gemm_quant_ws(Yd, Wd, Xd, T, out_f, in_f, dt) == NTK_E_SHAPE
    assert np.array_equal(Yd.numpy(np.uint32), before.view(np.uint32))


# ------------------------------------------------------------------------------- (4) ntk_embed_rows
@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("hidden", [32, 320, 864])
def test_embed_rows_bit_exact(qname, hidden):
    """row pitches of 34 / 340 / 918 and 18 / 180 / 486 bytes; first, last, a repeated and a middle row of 50"""
    dt = G.GGML_TO_DT[QUANT[qname]]
    vocab = 50
    r = rng(hidden, dt, 6)
    table = np.frombuffer(G.synth_tensor(r, QUANT[qname], vocab, hidden, sigma=20.0), np.uint8)
    toks = np.array([0, vocab - 1, 7, 7, 23], np.int32)
    ref = np.stack([O.embed_row(table, int(t), hidden, dt) for t in toks])
    od = DB.from_numpy(np.full(toks.size * hidden, np.nan, np.float32))
    ops.embed_rows(od, DB.from_numpy(table), DB.from_numpy(toks), toks.size, hidden, dt)
    got = od.numpy().reshape(toks.size, hidden)
    assert np.isfinite(got).all() and np.array_equal(got.view(np.uint32), ref.astype(np.float32).view(np.uint32))
