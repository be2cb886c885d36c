"""ntk_gemm_dense16 (csrc/gemm_dense16.hip): the prompt GEMM over unquantised F16 / BF16 rows on the 16-bit matrix cores, through the C ABI.

References: the float64 product over the EXACTLY widened matrix (half -> double, bfloat16 -> double are exact), and for up to 70 tokens the oracle's per-token
GEMV as in tests/test_gemv_dense16_gpu.py.  Bar: the project's tol_for(y, in) = 4e-6 sqrt(in) max(1, max |y|) (F32 sums in another order; the activations'
pieces are exact for BF16 and within one F32 ulp for F16).  The exactness tests need no bar: one non-zero activation per token against a power-of-two
weight has no rounding anywhere (BF16: three pieces spanning 24 bits; F16: the bound 2^-23 stated in csrc/gemm_f16.hip).

Run on the MI355X box:  python -m pytest tests/test_gemm_dense16_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from ntransformer_amd import gguf as G
from ntransformer_amd import ops
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O

pytestmark = pytest.mark.gpu

E_DTYPE, E_SHAPE, E_ALIGN = -1, -2, -4
FORMATS = {"F16": (G.GGML_F16, G.DT_F16), "BF16": (G.GGML_BF16, G.DT_BF16)}
GUARD = 4                                   # floats in front of and behind Y (Y stays 16-byte aligned)
BEHIND = 3                                  # rows of Y behind n_tokens
ALL_T = [1, 2, 15, 16, 17, 63, 64, 65, 70, 129]


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261021, seed]))


def tol_for(y, in_f):
    # (tests/test_hip_kernels.py, verbatim)
    return 4e-6 * np.sqrt(in_f) * max(1.0, float(np.abs(y).max()))


def widen(raw, fmt, out_f, in_f):
    """the matrix as float64, exactly"""
    w16 = raw.view("<u2")
    w = G.bf16_to_f32(w16) if fmt == "BF16" else w16.view(np.float16).astype(np.float32)
    return w.astype(np.float64).reshape(out_f, in_f)


def oracle_gemv(raw, fmt, out_f, in_f):
    if fmt == "BF16":
        wide = np.ascontiguousarray(G.bf16_to_f32(raw.view("<u2"))).view(np.uint8)
        return lambda x: O.gemv(wide, x, out_f, in_f, G.DT_F32)
    return lambda x: O.gemv(raw, x, out_f, in_f, G.DT_F16)


_CASES = {}


def case(fmt, out_f, in_f, n_tok=129):
    """matrix, token rows, residual rows, the float64 products and (first 70 tokens) the oracle's GEMVs: once per (format, shape), read-only"""
    key = (fmt, out_f, in_f, n_tok)
    if key not in _CASES:
        r = rng(out_f * 13 + in_f + int(FORMATS[fmt][1]))
        raw = np.frombuffer(G.synth_tensor(r, FORMATS[fmt][0], out_f, in_f), np.uint8)
        X = r.standard_normal((n_tok, in_f)).astype(np.float32)
        R = r.standard_normal((n_tok, out_f)).astype(np.float32)
        want = X.astype(np.float64) @ widen(raw, fmt, out_f, in_f).T
        gemv = oracle_gemv(raw, fmt, out_f, in_f)
        orc = np.stack([gemv(X[t]) for t in range(min(70, n_tok))]) if n_tok <= 129 else None
        for a in (X, R, want) + ((orc,) if orc is not None else ()):
            a.setflags(write=False)
        _CASES[key] = (raw, DB.from_numpy(raw), X, R, want, orc)
    return _CASES[key]


def launch(Wd, dt, X, out_f, in_f, resid=None, ws=None, reuse_x=0):
    """one matrix; Y sits inside a larger buffer: GUARD floats, T rows (the residual, or NaN), BEHIND rows, GUARD floats.  -> (status, Y rows, whole buffer before, after)"""
    T = X.shape[0]
    host = np.full(2 * GUARD + (T + BEHIND) * out_f, np.nan, np.float32)
    host[:GUARD] = -7.25
    host[-GUARD:] = 9.5
    body = host[GUARD:-GUARD].reshape(T + BEHIND, out_f)
    body[T:] = 123.5
    if resid is not None:
        body[:T] = resid
    buf = DB.from_numpy(host)
    y = buf.at(4 * GUARD)
    st = ops.gemm_dense16([(Wd, y, out_f, dt)], DB.from_numpy(X), T, in_f, resid=y if resid is not None else None, workspace=ws, reuse_x=reuse_x)
    got = buf.numpy(np.float32)
    return st, got[GUARD:-GUARD].reshape(T + BEHIND, out_f)[:T].copy(), host, got


def untouched_outside(host, got, T, out_f):
    keep = np.ones(len(host), bool)
    keep[GUARD:GUARD + T * out_f] = False
    return np.array_equal(host.view(np.uint32)[keep], got.view(np.uint32)[keep])


# ------------------------------------------------------------------------------------------------ random matrices
@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("out_f", [16, 48, 304])
@pytest.mark.parametrize("in_f", [32, 256, 2080, 4096])      # one step; 8; 65 (odd); 128
def test_random_matrices_meet_both_references(fmt, out_f, in_f):
    dt = FORMATS[fmt][1]
    raw, Wd, X, R, want, orc = case(fmt, out_f, in_f)
    worst64 = worst_orc = 0.0
    for T in ALL_T:
        for with_resid in (False, True):
            st, y, host, got = launch(Wd, dt, np.ascontiguousarray(X[:T]), out_f, in_f, resid=R[:T] if with_resid else None)
            assert st == 0, (T, with_resid, st)
            assert untouched_outside(host, got, T, out_f), (T, with_resid)      # rows behind T and the guard floats: their bit patterns
            assert np.isfinite(y).all(), (T, with_resid)
            add = R[:T].astype(np.float64) if with_resid else 0.0
            for t in range(T):
                ref = want[t] + (add[t] if with_resid else 0.0)
                bar = tol_for(ref, in_f)
                e = float(np.abs(y[t] - ref).max())
                worst64 = max(worst64, e / bar)
                assert e <= bar, (T, with_resid, t, e, bar)
                if T <= 70:
                    ref = orc[t] + (R[t] if with_resid else 0.0)
                    bar = tol_for(ref, in_f)
                    e = float(np.abs(y[t] - ref).max())
                    worst_orc = max(worst_orc, e / bar)
                    assert e <= bar, ("oracle", T, with_resid, t, e, bar)
    print("%s %dx%d: worst err / bar %.3f against float64, %.3f against the oracle's GEMV" % (fmt, out_f, in_f, worst64, worst_orc))


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_a_full_pass_of_1024_tokens(fmt):
    out_f, in_f, T = 48, 4096, 1024
    dt = FORMATS[fmt][1]
    raw, Wd, X, R, want, _ = case(fmt, out_f, in_f, n_tok=T)
    for with_resid in (False, True):
        st, y, host, got = launch(Wd, dt, X, out_f, in_f, resid=R if with_resid else None)
        assert st == 0 and untouched_outside(host, got, T, out_f) and np.isfinite(y).all()
        ref = want + (R.astype(np.float64) if with_resid else 0.0)
        bars = 4e-6 * np.sqrt(in_f) * np.maximum(1.0, np.abs(ref).max(axis=1))      # tol_for, per token row
        errs = np.abs(y - ref).max(axis=1)
        print("%s 48x4096 T=1024 resid=%d: worst err / bar %.3f" % (fmt, with_resid, float((errs / bars).max())))
        assert (errs <= bars).all()


# ------------------------------------------------------------------------------------------------ three segments
@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("rows,in_f", [((64, 16, 16), 256), ((4096, 1024, 1024), 4096)])
def test_three_segments_equal_their_one_segment_launches(fmt, rows, in_f):
    gt, dt = FORMATS[fmt]
    T = 17
    r = rng(sum(rows) + in_f + int(dt))
    Xd = DB.from_numpy(r.standard_normal((T, in_f)).astype(np.float32))
    Ws = [DB.from_numpy(np.frombuffer(G.synth_tensor(r, gt, n, in_f), np.uint8)) for n in rows]

    def fresh(n):
        return DB.from_numpy(np.full((T, n), np.nan, np.float32))

    together = [fresh(n) for n in rows]
    assert ops.gemm_dense16([(Ws[i], together[i], rows[i], dt) for i in range(3)], Xd, T, in_f) == 0
    for i in range(3):
        alone = fresh(rows[i])
        assert ops.gemm_dense16([(Ws[i], alone, rows[i], dt)], Xd, T, in_f) == 0
        a, b = together[i].numpy(np.uint32), alone.numpy(np.uint32)
        assert np.isfinite(alone.numpy(np.float32)).all() and np.array_equal(a, b), (fmt, rows, i)


# ------------------------------------------------------------------------------------------------ exactness
def pow2_matrix(r, fmt, out_f, in_f, lo, hi):
    """W[r, c] = +-2^e, e uniform in [lo, hi]: (raw bytes, float64 values)"""
    e = r.integers(lo, hi + 1, (out_f, in_f))
    sign = r.integers(0, 2, (out_f, in_f)).astype(np.uint16)
    if fmt == "BF16":
        bits = (sign << 15) | ((e + 127).astype(np.uint16) << 7)
    else:
        bits = (sign << 15) | ((e + 15).astype(np.uint16) << 10)
    vals = np.where(sign == 1, -1.0, 1.0) * np.exp2(e.astype(np.float64))
    return np.ascontiguousarray(bits.astype("<u2")).view(np.uint8).reshape(-1), vals


def full_mantissa(r, n, exp_lo=-4, exp_hi=4):
    """random F32 values whose 24-bit mantissa is used down to its last bit"""
    bits = (r.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)) | ((r.integers(exp_lo, exp_hi + 1, n) + 127).astype(np.uint32) << np.uint32(23)) | \
           r.integers(0, 1 << 23, n, dtype=np.uint32) | np.uint32(1)
    return bits.view(np.float32)


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_every_piece_of_an_activation_counts(fmt):
    """X is zero except one column per token; that column walks every position of two K steps and the last column.  A kernel that drops its last piece is
    off by 2^-17 (BF16) / 2^-12 (F16) of the product."""
    out_f, in_f = 16, 128
    dt = FORMATS[fmt][1]
    cols = list(range(64)) + [in_f - 1]
    T = len(cols)
    r = rng(700 + int(dt))
    raw, W = pow2_matrix(r, fmt, out_f, in_f, -8, 8)
    v = full_mantissa(r, T)
    X = np.zeros((T, in_f), np.float32)
    X[np.arange(T), cols] = v
    st, y, _, _ = launch(DB.from_numpy(raw), dt, X, out_f, in_f)
    assert st == 0
    want = v.astype(np.float64)[:, None] * W[:, cols].T                    # [T, out_f], exact in float64 and representable in F32
    if fmt == "BF16":
        assert np.array_equal(y.astype(np.float64), want)
    else:
        err = np.abs(y.astype(np.float64) - want)
        print("F16 one-column products: worst relative error 2^%.1f" % np.log2(max(float((err / np.abs(want)).max()), 2.0 ** -60)))
        assert (err <= 2.0 ** -23 * np.abs(want)).all()


def test_bf16_keeps_the_range_of_f32():
    """weights of 2^100 against activations of 2^-100 and the other way round: exact.  A kernel that narrowed BF16 to half would give Inf / 0."""
    out_f, in_f, T = 16, 32, 2
    r = rng(800)
    v = full_mantissa(r, T, 0, 0)
    for e in (100, -100):
        bits = np.full((out_f, in_f), (e + 127) << 7, "<u2")
        X = np.zeros((T, in_f), np.float32)
        X[0, 3] = v[0] * np.float32(2.0) ** -e
        X[1, 31] = v[1] * np.float32(2.0) ** -e
        assert X[0, 3] * np.float64(2.0) ** e == v[0]                      # (the scaling of the input is exact)
        st, y, _, _ = launch(DB.from_numpy(bits.view(np.uint8).reshape(-1)), G.DT_BF16, X, out_f, in_f)
        assert st == 0
        assert np.array_equal(y, np.repeat(v[:, None], out_f, axis=1)), e


def test_f16_subnormal_weights_are_kept():
    """W = 2^-24, the smallest FP16 subnormal: the matrix cores take it as it is"""
    out_f, in_f, T = 16, 32, 2
    v = full_mantissa(rng(801), T, 0, 0)
    bits = np.full((out_f, in_f), 1, "<u2")
    X = np.zeros((T, in_f), np.float32)
    X[0, 3], X[1, 31] = v
    st, y, _, _ = launch(DB.from_numpy(bits.view(np.uint8).reshape(-1)), G.DT_F16, X, out_f, in_f)
    assert st == 0
    want = np.repeat(v.astype(np.float64)[:, None], out_f, axis=1) * 2.0 ** -24
    assert (y != 0).all() and (np.abs(y.astype(np.float64) - want) <= 2.0 ** -23 * np.abs(want)).all()


# ------------------------------------------------------------------------------------------------ companions, determinism, reuse_x
@pytest.mark.parametrize("fmt", sorted(FORMATS))
@pytest.mark.parametrize("T", [17, 70])
def test_a_token_does_not_depend_on_its_companions(fmt, T):
    out_f, in_f = 48, 256
    dt = FORMATS[fmt][1]
    raw, Wd, X, _, _, _ = case(fmt, out_f, in_f)
    watched, sick = 5, T - 1
    _, y0, _, _ = launch(Wd, dt, np.ascontiguousarray(X[:T]), out_f, in_f)
    other = (37.0 * rng(900 + T).standard_normal((T, in_f))).astype(np.float32)
    other[watched] = X[watched]
    other[sick, 100] = np.nan
    st, y1, _, _ = launch(Wd, dt, other, out_f, in_f)
    assert st == 0
    assert np.array_equal(y0[watched].view(np.uint32), y1[watched].view(np.uint32))
    assert not np.isfinite(y1[sick]).any()
    healthy = [t for t in range(T) if t != sick]
    assert np.isfinite(y1[healthy]).all()


@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_three_launches_give_the_same_bits_and_reuse_x_too(fmt):
    out_f, in_f, T = 304, 2080, 70
    dt = FORMATS[fmt][1]
    raw, Wd, X, R, _, _ = case(fmt, out_f, in_f)
    x = np.ascontiguousarray(X[:T])
    runs = [launch(Wd, dt, x, out_f, in_f, resid=R[:T])[1] for _ in range(3)]
    assert np.array_equal(runs[0].view(np.uint32), runs[1].view(np.uint32)) and np.array_equal(runs[0].view(np.uint32), runs[2].view(np.uint32))
    # reuse_x = 1 behind a first call on the same workspace and the same X
    ws = ops.gemm_dense16_workspace(in_f, out_f, dt)
    Xd = DB.from_numpy(x)
    first = DB.from_numpy(np.full((T, out_f), np.nan, np.float32))
    again = DB.from_numpy(np.full((T, out_f), np.nan, np.float32))
    assert ops.gemm_dense16([(Wd, first, out_f, dt)], Xd, T, in_f, workspace=ws) == 0
    assert ops.gemm_dense16([(Wd, again, out_f, dt)], Xd, T, in_f, workspace=ws, reuse_x=1) == 0
    fresh = launch(Wd, dt, x, out_f, in_f)[1]
    assert np.array_equal(first.numpy(np.uint32), again.numpy(np.uint32))
    assert np.array_equal(again.numpy(np.uint32).reshape(T, out_f), fresh.view(np.uint32))


# ------------------------------------------------------------------------------------------------ refusals
@pytest.mark.parametrize("fmt", sorted(FORMATS))
def test_refusals_launch_nothing(fmt):
    gt, dt = FORMATS[fmt]
    other_dt = G.DT_BF16 if fmt == "F16" else G.DT_F16
    T, in_f, out_f = 17, 256, 64
    r = rng(1000 + int(dt))
    raw = np.frombuffer(G.synth_tensor(r, gt, out_f, in_f), np.uint8)
    Wd = DB(raw.nbytes + 64)
    Wd.upload(raw)
    Wd.upload(raw, 16)                                                     # (a second copy 16 bytes on: reads through W + 8 stay inside the buffer)
    Xd = DB.from_numpy(r.standard_normal((T + 1, in_f)).astype(np.float32))
    ws = ops.gemm_dense16_workspace(in_f, out_f, dt)
    poison = np.full((T + 1) * out_f + 8, np.nan, np.float32)
    poison[::3] = -1.5

    def refused(want, segs_of, X=Xd.ptr, n_in=in_f, resid_off=None, ws_off=0, repacked=False):
        y = DB.from_numpy(poison)
        segs = segs_of(y)
        st = ops.gemm_dense16(segs, X, T, n_in, resid=None if resid_off is None else y.at(resid_off), workspace=ws.at(ws_off), repacked=repacked)
        assert st == want, (st, want)
        assert np.array_equal(y.numpy(np.uint32), poison.view(np.uint32))

    refused(E_SHAPE, lambda y: [(Wd, y, 24, dt)])                                      # rows % 16
    refused(E_SHAPE, lambda y: [(Wd, y, 32, dt), (Wd, y.at(4 * T * 32), 8, dt)])
    refused(E_SHAPE, lambda y: [(Wd, y, out_f, dt)], n_in=48)                          # in_features % 32
    refused(E_SHAPE, lambda y: [(Wd, y, out_f, dt)], n_in=264)
    refused(E_SHAPE, lambda y: [(Wd, y, out_f, dt)], repacked=True)                    # weights_repacked must be 0
    refused(E_SHAPE, lambda y: [(Wd, y, 32, dt), (Wd, y.at(4 * T * 32), 32, dt)], resid_off=0)   # a residual with two matrices
    refused(E_ALIGN, lambda y: [(Wd.at(8), y, out_f, dt)])                             # W
    refused(E_ALIGN, lambda y: [(Wd, y.at(4), out_f, dt)])                             # Y
    refused(E_ALIGN, lambda y: [(Wd, y, out_f, dt)], X=Xd.at(4))                       # X
    refused(E_ALIGN, lambda y: [(Wd, y, out_f, dt)], resid_off=8)                      # resid
    refused(E_ALIGN, lambda y: [(Wd, y, out_f, dt)], ws_off=8)                         # workspace
    refused(E_DTYPE, lambda y: [(Wd, y, out_f, G.DT_Q8_0)])                            # not a 16-bit dtype
    refused(E_DTYPE, lambda y: [(Wd, y, out_f, G.DT_F32)])
    refused(E_DTYPE, lambda y: [(Wd, y, 32, dt), (Wd, y.at(4 * T * 32), 32, other_dt)])   # mixed segments
    refused(E_DTYPE, lambda y: [(Wd, y, 32, other_dt), (Wd, y.at(4 * T * 32), 16, dt), (Wd, y.at(4 * T * 48), 16, dt)])
