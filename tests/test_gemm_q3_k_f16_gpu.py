"""GPU tests of Q3_K on the FP16 matrix-core prompt GEMM (csrc/gemm_f16.hip: DeqI<Q3_K> over the GGUF blocks, DeqI<Q3_K + GB_RP> over the decode repack), in
each of its three kernel forms (the form a case takes is asserted from the launch's own plan, ntk_gemm_quant_f16_form): the raw form against the float64
product X . W^T for W = gguf.dequantize(...), per token at the bar of every other format of this GEMM (tests/test_hip_kernels.py: 4e-6 sqrt(in) max(1, |y|max));
the repack form against the raw form bit for bit; the refusals the engine's fallback relies on.  Token rows carry scales over e^+-3, an outlier channel and
an all-zero super-block; every output starts as NaN.
Run on the MI355X box:  python -m pytest tests/test_gemm_q3_k_f16_gpu.py -m gpu -x -q -s"""
import ctypes as C

import numpy as np
import pytest

from ntransformer_amd import _lib, gguf as G, ops
from ntransformer_amd.ops import DeviceBuffer as DB

pytestmark = pytest.mark.gpu
Q3, Q4, DT = G.GGML_Q3_K, G.GGML_Q4_K, G.GGML_TO_DT
E_DTYPE, E_SHAPE = -1, -2
FORMS = ("K-slice", "small", "chunk")

# case: (tokens, rows of the launch's matrices, columns, residual in place, the form and rows per wave the plan takes)
CASES = {
    "3x16x256": (3, (16,), 256, False, "small", 16),              # one unit, even parity only (a single unit is no K slice: the weight-streaming form)
    "16x32x1024": (16, (32,), 1024, False, "K-slice", 16),        # the K-slice form; units of odd parity under the aligned form
    "20x48x512": (20, (48,), 512, False, "small", 16),            # two token blocks (no K-slice form for a per-16-column format); an odd-parity unit
    "33x48x768": (33, (48,), 768, False, "chunk", 16),            # the first token count past the short forms; 330-byte rows: the AL = false form
    "70x272x1024": (70, (272,), 1024, False, "chunk", 16),        # two 64-token chunks, the second ragged; a last workgroup of one 16-row tile
    "130x32x4096": (130, (32,), 4096, False, "chunk", 16),        # a K split of 8
    "70x272x1024+resid": (70, (272,), 1024, True, "chunk", 16),   # the residual epilogue, in place (behind a K split)
    "20x48|32x512": (20, (48, 32), 512, False, "small", 16),      # two Q3_K matrices in one launch
    "16x48|32x512": (16, (48, 32), 512, False, "K-slice", 16),    # ... in the K-slice form
    "40x1040|1024x512": (40, (1040, 1024), 512, False, "chunk", 32),   # 32 rows per wave (2048 rows and more), the first matrix not in whole 128-row tiles
}


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)


def tol_for(y, in_f):
    return 4e-6 * np.sqrt(in_f) * max(1.0, float(np.abs(y).max()))


def form_of(segs, X, T, in_f, repacked):   # what ntk_gemm_quant_f16 plans for these matrices: (form, rows per wave)
    arr = (ops.GemvSeg * len(segs))()
    for i, (W, y, rows, dt) in enumerate(segs): arr[i].W, arr[i].y, arr[i].rows, arr[i].dtype = W.ptr, y.ptr, rows, int(dt)
    d, rpw = _lib.GemmDesc(), C.c_int(0)
    d.segs, d.nseg, d.X, d.n_tokens, d.in_features, d.workspace, d.weights_repacked = arr, len(segs), X.ptr, T, in_f, X.ptr, int(repacked)
    f = _lib.lib().ntk_gemm_quant_f16_form(C.byref(d), C.byref(rpw))
    return FORMS[f] if f >= 0 else f, rpw.value


@pytest.mark.parametrize("case", sorted(CASES))
def test_raw_form_meets_the_float64_product_and_the_repack_form_its_bits(case):
    T, rows, in_f, resid, form, rpw = CASES[case]
    r = np.random.Generator(np.random.Philox(key=[20261126, T + sum(rows) + in_f]))
    raws = [np.frombuffer(G.synth_tensor(r, Q3, o, in_f), np.uint8) for o in rows]
    X = r.standard_normal((T, in_f)) * np.exp(r.uniform(-3, 3, (T, 1)))
    X[:, 5] *= 300.0                        # an outlier channel
    if in_f >= 512: X[:, 256:512] = 0.0     # an all-zero super-block
    X = X.astype(np.float32)
    start = [r.standard_normal((T, o)).astype(np.float32) if resid else np.full((T, o), np.nan, np.float32) for o in rows]
    Xd, got = DB.from_numpy(X), {}
    for repacked in (False, True):
        Ws = [DB.from_numpy(w) for w in raws]
        if repacked: Ws = [ops.rp_pack(W, o, in_f, DT[Q3]) for W, o in zip(Ws, rows)]
        ys = [DB.from_numpy(s) for s in start]
        segs = [(W, y, o, DT[Q3]) for W, y, o in zip(Ws, ys, rows)]
        assert form_of(segs, Xd, T, in_f, repacked) == (form, rpw)
        assert ops._gemm_quant_f16(segs, Xd, T, in_f, resid=ys[0] if resid else None, repacked=repacked) == 0
        got[repacked] = [y.numpy(np.float32).reshape(T, o) for y, o in zip(ys, rows)]
    refs = [X.astype(np.float64) @ G.dequantize(w, Q3, o * in_f).astype(np.float64).reshape(o, in_f).T + (s if resid else 0.0) for w, o, s in zip(raws, rows, start)]
    worst = max(float(np.abs(y[t] - ref[t]).max()) / tol_for(ref[t], in_f) for y, ref in zip(got[False], refs) for t in range(T))
    print("Q3_K %s: the %s form, %d rows per wave: worst error / bound over the tokens = %.3g" % (case, form, rpw, worst))
    assert all(np.isfinite(y).all() for y in got[False]) and worst <= 1.0
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got[False], got[True]))


@pytest.mark.parametrize("what", ["128 columns", "24 rows", "Q3_K with Q4_K"])
@pytest.mark.parametrize("repacked", [False, True])
def test_refusals_write_nothing(what, repacked, T=20):
    rows, in_f, dts = {"128 columns": ((16,), 128, (Q3,)), "24 rows": ((24,), 256, (Q3,)), "Q3_K with Q4_K": ((16, 16), 256, (Q3, Q4))}[what]
    W, Xd = DB.zeros(1 << 16), DB.from_numpy(np.ones((T, in_f), np.float32))
    ys = [DB.from_numpy(np.full((T, o), np.nan, np.float32)) for o in rows]
    st = ops.gemm_quant_ws_multi([(W, y, o, DT[gt]) for y, o, gt in zip(ys, rows, dts)], Xd, T, in_f, repacked=repacked)
    assert st in (E_SHAPE, E_DTYPE), st
    assert all(np.isnan(y.numpy(np.float32)).all() for y in ys)
