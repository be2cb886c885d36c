"""GPU tests of IQ4_NL and IQ4_XS on the FP16 matrix-core prompt GEMM (csrc/gemm_f16.hip: DeqI<IQ4_NL>, DeqI<IQ4_XS> over the GGUF blocks, DeqI<IQ4_XS + GB_RP>
over the decode repack): the raw form against the float64 product X . W^T for W = gguf.dequantize(...), per token at the bar of every other format of this
GEMM (tests/test_hip_kernels.py: 4e-6 sqrt(in) max(1, |y|max)); for IQ4_XS the repack form against the raw form bit for bit; the refusals the engine's
fallback relies on.  Token rows carry scales over e^+-3, an outlier channel and an all-zero super-block; every output starts as NaN.  The form each case takes
is read from the launch's own plan (ntk_gemm_quant_f16_form) and printed; over the list each type meets all three forms.  The 2-byte aligned form (AL =
false) cannot be reached by either type: whole units need in_features % 256 == 0, which puts every IQ4_NL row on 16 bytes, and IQ4_XS rows are multiples of
136 bytes at any width -- so it is not tested.
Run on the MI355X box:  python -m pytest tests/test_gemm_iq4_f16_gpu.py -m gpu -x -q -s"""
import ctypes as C

import numpy as np
import pytest

from ntransformer_amd import _lib, gguf as G, ops
from ntransformer_amd.ops import DeviceBuffer as DB

pytestmark = pytest.mark.gpu
TYPES = {"IQ4_NL": G.GGML_IQ4_NL, "IQ4_XS": G.GGML_IQ4_XS}
Q4, DT = G.GGML_Q4_K, G.GGML_TO_DT
E_DTYPE, E_SHAPE = -1, -2
FORMS = ("K-slice", "small", "chunk")

# case: (tokens, rows of the launch's matrices, columns, residual in place)
CASES = {
    "3x16x256": (3, (16,), 256, False),               # one unit; IQ4_XS: a row pitch of 136, so the rows' windows alternate shift 0 / 8
    "16x32x1024": (16, (32,), 1024, False),           # the K-slice form, units of both parities
    "20x48x768": (20, (48,), 768, False),             # the first token count past the K-slice limit; an odd super-block count: shift 8 on odd rows; three units
    "70x272x1024": (70, (272,), 1024, False),         # two 64-token chunks, the second ragged; a last workgroup of one 16-row tile
    "130x32x4096": (130, (32,), 4096, False),         # a K split
    "70x272x1024+resid": (70, (272,), 1024, True),    # the residual epilogue, in place
    "16x48|32x512": (16, (48, 32), 512, False),       # two matrices of the type in one launch
    "40x1040|1024x512": (40, (1040, 1024), 512, False),   # ... at 32 rows per wave (2048 rows and more), the first matrix not in whole 128-row tiles
}

@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)

def form_of(segs, X, T, in_f, repacked):   # what ntk_gemm_quant_f16 plans for these matrices: (form, rows per wave)
    arr = (ops.GemvSeg * len(segs))()
    for i, (W, y, rows, dt) in enumerate(segs): arr[i].W, arr[i].y, arr[i].rows, arr[i].dtype = W.ptr, y.ptr, rows, int(dt)
    d, rpw = _lib.GemmDesc(), C.c_int(0)
    d.segs, d.nseg, d.X, d.n_tokens, d.in_features, d.workspace, d.weights_repacked = arr, len(segs), X.ptr, T, in_f, X.ptr, int(repacked)
    f = _lib.lib().ntk_gemm_quant_f16_form(C.byref(d), C.byref(rpw))
    return FORMS[f] if f >= 0 else f, rpw.value

@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("name", sorted(TYPES))
def test_raw_form_meets_the_float64_product_and_the_repack_form_its_bits(name, case):
    gt, (T, rows, in_f, resid) = TYPES[name], CASES[case]
    r = np.random.Generator(np.random.Philox(key=[20261126, T + sum(rows) + in_f]))
    raws = [np.frombuffer(G.synth_tensor(r, gt, o, in_f), np.uint8) for o in rows]
    X = r.standard_normal((T, in_f)) * np.exp(r.uniform(-3, 3, (T, 1)))
    X[:, 5] *= 300.0                        # an outlier channel
    if in_f >= 512: X[:, 256:512] = 0.0     # an all-zero super-block
    X = X.astype(np.float32)
    start = [r.standard_normal((T, o)).astype(np.float32) if resid else np.full((T, o), np.nan, np.float32) for o in rows]
    Xd, got, forms = DB.from_numpy(X), {}, {}
    for repacked in (False, True) if name == "IQ4_XS" else (False,):   # (IQ4_NL has no repack)
        Ws = [DB.from_numpy(w) for w in raws]
        if repacked: Ws = [ops.rp_pack(W, o, in_f, DT[gt]) for W, o in zip(Ws, rows)]
        ys = [DB.from_numpy(s) for s in start]
        segs = [(W, y, o, DT[gt]) for W, y, o in zip(Ws, ys, rows)]
        forms[repacked] = form_of(segs, Xd, T, in_f, repacked)
        assert ops._gemm_quant_f16(segs, Xd, T, in_f, resid=ys[0] if resid else None, repacked=repacked) == 0
        got[repacked] = [y.numpy(np.float32).reshape(T, o) for y, o in zip(ys, rows)]
    refs = [X.astype(np.float64) @ G.dequantize(w, gt, o * in_f).astype(np.float64).reshape(o, in_f).T + (s if resid else 0.0) for w, o, s in zip(raws, rows, start)]
    tol = lambda y: 4e-6 * np.sqrt(in_f) * max(1.0, float(np.abs(y).max()))   # per token: the bar of every format of this GEMM
    worst = max(float(np.abs(y[t] - ref[t]).max()) / tol(ref[t]) for y, ref in zip(got[False], refs) for t in range(T))
    print("%s %s: the %s form, %d rows per wave: worst error / bound over the tokens = %.3g" % ((name, case) + forms[False] + (worst,)))
    assert forms[False][0] in FORMS and all(f == forms[False] for f in forms.values())
    assert all(np.isfinite(y).all() for y in got[False]) and worst <= 1.0
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(got[False], got.get(True, got[False])))

@pytest.mark.parametrize("name", sorted(TYPES))
def test_the_cases_take_each_of_the_three_forms(name):
    buf = DB.zeros(16)   # (the plan reads no memory: any non-null pointers)
    took = {form_of([(buf, buf, o, DT[TYPES[name]]) for o in rows], buf, T, in_f, False)[0] for T, rows, in_f, _ in CASES.values()}
    assert took == set(FORMS), took

@pytest.mark.parametrize("what", ["IQ4_NL repacked", "IQ4_XS with Q4_K", "24 rows"])
def test_refusals_write_nothing(what, T=20):
    XS, NL = TYPES["IQ4_XS"], TYPES["IQ4_NL"]
    rows, dts, repacked = {"IQ4_NL repacked": ((16,), (NL,), True), "IQ4_XS with Q4_K": ((16, 16), (XS, Q4), False), "24 rows": ((24,), (XS,), False)}[what]
    W, Xd = DB.zeros(1 << 16), DB.from_numpy(np.ones((T, 256), np.float32))
    ys = [DB.from_numpy(np.full((T, o), np.nan, np.float32)) for o in rows]
    st = ops.gemm_quant_ws_multi([(W, y, o, DT[gt]) for y, o, gt in zip(ys, rows, dts)], Xd, T, 256, repacked=repacked)
    assert st in (E_SHAPE, E_DTYPE), st
    assert all(np.isnan(y.numpy(np.float32)).all() for y in ys)
