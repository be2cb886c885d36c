"""The kernels of the unquantised 16-bit formats (IEEE half, bfloat16) against the oracle: ntk_gemv / ntk_embed_rows with NTK_DT_BF16, the fused decode GEMV
of csrc/gemv_dense16.hip behind ntk_gemv_fused in its four forms, and the F32-MFMA prompt GEMM (ntk_gemm_quant) with 16-bit rows.

Reference: a bfloat16 weight IS a float (its bits are the high half), so the oracle's F32 GEMV over the widened matrix is the BF16 reference with no quantiser
in between; the F16 reference is the oracle's F16 GEMV.  Bars: tol_for of tests/test_hip_kernels.py (F32 sums in another order), times 2 behind a fused
RMSNorm / for three segments and times 4 for SiLU(gate) x up -- the bars the quantised forms have.

Run on the MI355X box:  python -m pytest tests/test_gemv_dense16_gpu.py -m gpu -x -q"""
import ctypes as C

import numpy as np
import pytest

from ntransformer_amd import gguf as G
from ntransformer_amd import _lib, ops
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O

pytestmark = pytest.mark.gpu

E_DTYPE, E_ALIGN = -1, -4
FORMATS = {"F16": (G.GGML_F16, G.DT_F16), "BF16": (G.GGML_BF16, G.DT_BF16)}
EPS = 1e-5


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261020, seed]))


def tol_for(y, in_f):
    # (tests/test_hip_kernels.py, verbatim) F32 accumulation in a different association order than the oracle: error ~ eps * sqrt(in) * |terms|
    return 4e-6 * np.sqrt(in_f) * max(1.0, float(np.abs(y).max()))


def matrix(r, fmt, out_f, in_f):
    """(raw bytes, reference(x) -> the oracle's GEMV): BF16 through the widened F32 matrix, F16 through the oracle's own F16 path"""
    gt, dt = FORMATS[fmt]
    raw = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    if fmt == "BF16":
        wide = np.ascontiguousarray(G.bf16_to_f32(raw.view("<u2"))).view(np.uint8)
        return raw, (lambda x: O.gemv(wide, x, out_f, in_f, G.DT_F32))
    return raw, (lambda x: O.gemv(raw, x, out_f, in_f, G.DT_F16))


def rmsnorm(x, w):
    return O.rmsnorm(x[None, :], w, EPS)[0]


def fused_status(segs, x, in_f, norm_w=None, resid=None, silu_pair=False):
    arr = (_lib.GemvSeg * len(segs))()
    for i, (W, y, rows, dt) in enumerate(segs):
        arr[i].W, arr[i].y, arr[i].rows, arr[i].dtype = ops._p(W), ops._p(y), rows, int(dt)
    st = _lib.lib().ntk_gemv_fused(arr, len(segs), ops._p(x), in_f, ops._p(norm_w), EPS, ops._p(resid), int(silu_pair), None)
    ops.synchronize()
    return st


# ------------------------------------------------------------------------------------------------ the 1:1 operators
@pytest.mark.parametrize("in_f", [3, 8, 100, 264, 4096])
def test_gemv_bf16(in_f):
    out_f = 45
    r = rng(in_f)
    raw, ref = matrix(r, "BF16", out_f, in_f)
    x = r.standard_normal(in_f).astype(np.float32)
    want = ref(x)
    Wd, xd = DB.from_numpy(raw), DB.from_numpy(x)
    yd = DB.from_numpy(np.full(out_f, np.nan, np.float32))
    ops.launch_gemv(yd, Wd, xd, out_f, in_f, G.DT_BF16)
    y = yd.numpy(np.float32)
    err = float(np.abs(y - want).max())
    print("ntk_gemv BF16 in=%d: err %.3g, bar %.3g" % (in_f, err, tol_for(want, in_f)))
    assert np.isfinite(y).all() and err <= tol_for(want, in_f)


def test_gemv_add_stays_f16_only():
    d = DB.zeros(4096)
    assert _lib.lib().ntk_gemv_add(d.ptr, d.ptr, d.ptr, 4, 8, G.DT_BF16, None) == E_DTYPE


def test_embed_rows_bf16_is_the_widened_table():
    hidden, vocab = 264, 37
    r = rng(77)
    raw = np.frombuffer(G.synth_tensor(r, G.GGML_BF16, vocab, hidden), np.uint8)
    table = G.bf16_to_f32(raw.view("<u2")).reshape(vocab, hidden)
    toks = np.array([0, 36, 5, 5, 17], np.int32)
    out = DB.from_numpy(np.full((len(toks), hidden), np.nan, np.float32))
    ops.embed_rows(out, DB.from_numpy(raw), DB.from_numpy(toks), len(toks), hidden, G.DT_BF16)
    got = out.numpy(np.float32).reshape(len(toks), hidden)
    assert np.array_equal(got.view(np.uint32), table[toks].view(np.uint32))


# ------------------------------------------------------------------------------------------------ the fused decode GEMV
SHAPES = [(1, 8), (45, 264), (300, 4096), (257, 14336)]


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("out_f,in_f", SHAPES)
def test_fused_plain_norm_and_residual(fmt, out_f, in_f):
    dt = FORMATS[fmt][1]
    r = rng(out_f * 3 + in_f + dt)
    raw, ref = matrix(r, fmt, out_f, in_f)
    x = r.standard_normal(in_f).astype(np.float32)
    nw = (1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32)
    res = r.standard_normal(out_f).astype(np.float32)
    Wd, xd, nwd = DB.from_numpy(raw), DB.from_numpy(x), DB.from_numpy(nw)
    plain, normed = ref(x), ref(rmsnorm(x, nw))

    def run(**kw):
        yd = DB.from_numpy(np.full(out_f, np.nan, np.float32))
        assert fused_status([(Wd, yd, out_f, dt)], xd, in_f, **kw) == 0
        return yd.numpy(np.float32)

    y = run()
    e = float(np.abs(y - plain).max())
    print("%s %dx%d plain: err %.3g, bar %.3g" % (fmt, out_f, in_f, e, tol_for(plain, in_f)))
    assert np.isfinite(y).all() and e <= tol_for(plain, in_f)
    assert np.array_equal(y, run())                                    # two launches of one call: the same bits
    y = run(norm_w=nwd)
    e = float(np.abs(y - normed).max())
    print("%s %dx%d norm: err %.3g, bar %.3g" % (fmt, out_f, in_f, e, 2 * tol_for(normed, in_f)))
    assert np.isfinite(y).all() and e <= 2 * tol_for(normed, in_f)
    assert np.array_equal(y, run(norm_w=nwd))
    # residual in place, inside a larger buffer whose other bytes must stay as they are
    pad = 5
    host = np.full(out_f + 2 * pad, np.nan, np.float32)
    host[pad:pad + out_f] = res
    host[:pad] = -7.25
    host[pad + out_f:] = 9.5
    buf = DB.from_numpy(host)
    # (y 16-byte alignment is not required: rows are stored one float at a time)
    assert fused_status([(Wd, buf.at(4 * pad), out_f, dt)], xd, in_f, resid=buf.at(4 * pad)) == 0
    got = buf.numpy(np.float32)
    want = res + plain
    e = float(np.abs(got[pad:pad + out_f] - want).max())
    print("%s %dx%d residual: err %.3g, bar %.3g" % (fmt, out_f, in_f, e, tol_for(want, in_f)))
    assert e <= tol_for(want, in_f)
    assert np.array_equal(got[:pad].view(np.uint32), host[:pad].view(np.uint32)) and np.array_equal(got[pad + out_f:].view(np.uint32), host[pad + out_f:].view(np.uint32))


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("rows,in_f", [((64, 16, 16), 264), ((4096, 1024, 1024), 4096)])
def test_fused_three_segments(fmt, rows, in_f):
    dt = FORMATS[fmt][1]
    r = rng(sum(rows) + in_f + dt)
    x = r.standard_normal(in_f).astype(np.float32)
    nw = (1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32)
    xn = rmsnorm(x, nw)
    mats = [matrix(r, fmt, n, in_f) for n in rows]
    Wd = [DB.from_numpy(m[0]) for m in mats]
    xd, nwd = DB.from_numpy(x), DB.from_numpy(nw)

    def run():
        ys = [DB.from_numpy(np.full(n, np.nan, np.float32)) for n in rows]
        assert fused_status([(Wd[i], ys[i], rows[i], dt) for i in range(3)], xd, in_f, norm_w=nwd) == 0
        return [y.numpy(np.float32) for y in ys]

    got, again = run(), run()
    for i in range(3):
        want = mats[i][1](xn)
        e = float(np.abs(got[i] - want).max())
        print("%s Q|K|V segment %d (%d rows, in %d): err %.3g, bar %.3g" % (fmt, i, rows[i], in_f, e, 2 * tol_for(want, in_f)))
        assert np.isfinite(got[i]).all() and e <= 2 * tol_for(want, in_f)
        assert np.array_equal(got[i], again[i])


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("in_f,inter", [(256, 512), (4096, 1792), (4096, 14336)])
def test_fused_silu_pair(fmt, in_f, inter):
    dt = FORMATS[fmt][1]
    r = rng(in_f + inter + dt)
    x = r.standard_normal(in_f).astype(np.float32)
    nw = (1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32)
    xn = rmsnorm(x, nw)
    (graw, gref), (uraw, uref) = matrix(r, fmt, inter, in_f), matrix(r, fmt, inter, in_f)
    g, u = gref(xn), uref(xn)
    want = O.silu_mul(g, u)
    Gd, Ud, xd, nwd = DB.from_numpy(graw), DB.from_numpy(uraw), DB.from_numpy(x), DB.from_numpy(nw)

    def run():
        yg = DB.from_numpy(np.full(inter, np.nan, np.float32))
        yu = DB.from_numpy(np.full(inter, np.nan, np.float32))
        assert fused_status([(Gd, yg, inter, dt), (Ud, yu, inter, dt)], xd, in_f, norm_w=nwd, silu_pair=True) == 0
        return yg.numpy(np.float32)

    y = run()
    bar = 4 * tol_for(np.concatenate([g, u, want]), in_f)
    e = float(np.abs(y - want).max())
    print("%s gate|up %d -> %d: err %.3g, bar %.3g" % (fmt, in_f, inter, e, bar))
    assert np.isfinite(y).all() and e <= bar
    assert np.array_equal(y, run())


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_fused_unaligned_shapes_are_left_to_the_caller(fmt):
    """The fallback this library chose: in_features that is no multiple of 8, or a weight / x pointer off the 16-byte grid, is NTK_E_ALIGN -- nothing is
    launched, y keeps its bytes -- and the 1:1 sequence (ntk_gemv: its dense kernel has a scalar path) computes the same shape within the bar."""
    dt = FORMATS[fmt][1]
    out_f = 45
    r = rng(100 + dt)
    for in_f, w_off, x_off in ((100, 0, 0), (264, 2, 0), (264, 0, 4)):
        raw, ref = matrix(r, fmt, out_f, in_f)
        x = r.standard_normal(in_f).astype(np.float32)
        Wd = DB(raw.nbytes + 64)
        Wd.upload(raw, w_off)
        xd = DB(x.nbytes + 64)
        xd.upload(x, x_off)
        poison = np.full(out_f, np.nan, np.float32)
        yd = DB.from_numpy(poison)
        assert fused_status([(Wd.at(w_off), yd, out_f, dt)], xd.at(x_off), in_f) == E_ALIGN
        assert np.array_equal(yd.numpy(np.uint32), poison.view(np.uint32))
        ops.launch_gemv(yd, Wd.at(w_off), xd.at(x_off), out_f, in_f, dt)
        want = ref(x)
        assert float(np.abs(yd.numpy(np.float32) - want).max()) <= tol_for(want, in_f)


def test_fused_mixed_16_bit_formats_are_not_taken():
    out_f, in_f = 16, 264
    r = rng(5)
    a, _ = matrix(r, "F16", out_f, in_f)
    b, _ = matrix(r, "BF16", out_f, in_f)
    x = DB.from_numpy(r.standard_normal(in_f).astype(np.float32))
    poison = np.full(out_f, np.nan, np.float32)
    ya, yb = DB.from_numpy(poison), DB.from_numpy(poison)
    Ad, Bd = DB.from_numpy(a), DB.from_numpy(b)
    for segs in ([(Ad, ya, out_f, G.DT_F16), (Bd, yb, out_f, G.DT_BF16)], [(Bd, yb, out_f, G.DT_BF16), (Ad, ya, out_f, G.DT_F16)],
                 [(Bd, yb, out_f, G.DT_BF16), (Ad, ya, out_f, G.DT_Q8_0)]):
        assert fused_status(segs, x, in_f) == E_DTYPE                      # the code the engine's not_taken() recognises
        assert np.array_equal(ya.numpy(np.uint32), poison.view(np.uint32)) and np.array_equal(yb.numpy(np.uint32), poison.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the prompt GEMM
_GEMM_CACHE = {}


def gemm_case(fmt, out_f, in_f):
    """matrix, 70 token rows and their per-token oracle results: computed once per (format, shape), shared by the T / residual cases, never written to"""
    key = (fmt, out_f, in_f)
    if key not in _GEMM_CACHE:
        r = rng(out_f * 11 + in_f + FORMATS[fmt][1])
        raw, ref = matrix(r, fmt, out_f, in_f)
        X = r.standard_normal((70, in_f)).astype(np.float32)
        R = r.standard_normal((70, out_f)).astype(np.float32)
        want = np.stack([ref(X[t]) for t in range(70)])
        for a in (X, R, want):
            a.setflags(write=False)
        _GEMM_CACHE[key] = (raw, X, R, want)
    return _GEMM_CACHE[key]


@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("out_f,in_f", [(64, 256), (300, 4096), (96, 2080)])
@pytest.mark.parametrize("T", [2, 17, 70])
@pytest.mark.parametrize("with_resid", [False, True])
def test_gemm_quant_16_bit_rows(fmt, out_f, in_f, T, with_resid):
    dt = FORMATS[fmt][1]
    raw, X, R, want = gemm_case(fmt, out_f, in_f)
    behind = 3                                                            # rows behind T: must stay untouched
    host = np.full((T + behind, out_f), np.nan, np.float32)
    if with_resid:
        host[:T] = R[:T]
    host[T:] = 123.5
    Yd = DB.from_numpy(host)
    ops.gemm_quant(Yd, DB.from_numpy(raw), DB.from_numpy(np.ascontiguousarray(X[:T])), T, out_f, in_f, dt, resid=Yd if with_resid else None)
    ops.synchronize()
    got = Yd.numpy(np.float32).reshape(T + behind, out_f)
    ref = want[:T] + (R[:T] if with_resid else 0.0)
    assert np.isfinite(got[:T]).all()
    worst = 0.0
    for t in range(T):                                                    # every token row against ITS oracle GEMV and its own bar
        e = float(np.abs(got[t] - ref[t]).max())
        worst = max(worst, e / tol_for(ref[t], in_f))
        assert e <= tol_for(ref[t], in_f), (t, e, tol_for(ref[t], in_f))
    print("%s gemm %dx%d T=%d resid=%d: worst err / bar %.3f" % (fmt, out_f, in_f, T, with_resid, worst))
    assert np.array_equal(got[T:].view(np.uint32), host[T:].view(np.uint32))


def test_gemm_quant_16_bit_rows_need_an_aligned_matrix():
    raw, X, _, _ = gemm_case("BF16", 64, 256)
    Wd = DB(raw.nbytes + 64)
    Wd.upload(raw, 2)
    poison = np.full((2, 64), np.nan, np.float32)
    Yd = DB.from_numpy(poison)
    st = _lib.lib().ntk_gemm_quant(Yd.ptr, Wd.at(2), DB.from_numpy(np.ascontiguousarray(X[:2])).ptr, 2, 64, 256, G.DT_BF16, None, None)
    ops.synchronize()
    assert st == E_ALIGN and np.array_equal(Yd.numpy(np.uint32), poison.view(np.uint32).reshape(-1))
