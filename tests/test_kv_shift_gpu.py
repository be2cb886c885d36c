"""The context shift kernels (csrc/kv_ops.hip: ntk_kv_shift, ntk_kv_shift_q8) on the GPU against the numpy checkers of ntransformer_amd/kv_ops.py:
K rows rotated to their new positions, V rows bit for bit, every byte outside the destination rows unchanged -- disjoint and overlapping moves, both
pairings, both cache formats.

Run on the MI355X box:  python -m pytest tests/test_kv_shift_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from ntransformer_amd import kv_ops as KO
from ntransformer_amd import kv_q8, ops
from ntransformer_amd.ops import DeviceBuffer as DB

pytestmark = pytest.mark.gpu
THETA = 500000.0
L, S, NKV = 2, 96, 2
# (src0, dst0, n_rows): one row; disjoint; overlapping, ten steps' worth of rows; one position down, up to the last row of the buffer
CASES = [(1, 0, 1), (50, 3, 10), (8, 4, 40), (33, 32, 63)]
NTK_E_SHAPE, NTK_E_NULL = -2, -5


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261019, seed]))


def table(hd):
    """an explicit F32 frequency table: the checker and the kernel read the same floats"""
    return KO.pair_freqs(hd, THETA)


_f16 = {}


def f16_caches(hd):
    """random unit-variance F16 caches [L][S][NKV * hd] (computed once per head size, never modified)"""
    if hd not in _f16:
        r = rng(hd)
        k = r.standard_normal((L, S, NKV * hd)).astype(np.float16).view(np.uint16)
        v = r.standard_normal((L, S, NKV * hd)).astype(np.float16).view(np.uint16)
        k.setflags(write=False)
        v.setflags(write=False)
        _f16[hd] = (k, v)
    return _f16[hd]


_q8 = []


def q8_caches():
    """random unit-variance 8-bit caches as canonical blocks [L][S][NKV * 128 / 32][34] (computed once)"""
    if not _q8:
        r = rng(7)
        kb = kv_q8.to_blocks(*kv_q8.quantize_q8_0(r.standard_normal((L, S, NKV * 128)).astype(np.float32)))
        vb = kv_q8.to_blocks(*kv_q8.quantize_q8_0(r.standard_normal((L, S, NKV * 128)).astype(np.float32)))
        kb.setflags(write=False)
        vb.setflags(write=False)
        _q8.extend([kb, vb])
    return _q8


# ------------------------------------------------------------------------------------------------ F16
@pytest.mark.parametrize("src0,dst0,n", CASES)
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
def test_kv_shift_f16_against_the_checker(hd, interleaved, src0, dst0, n):
    """K within one half rounding at the pair's magnitude of shift_f16_ref -- 2^-10 max(|a|, |b|) + 2^-24 per element, over an F32 error a thousand
    times smaller --, V rows bit for bit, every byte of both whole buffers outside the destination rows unchanged.
    (Where kernel and checker round a value to different neighbouring halves they differ by one ulp of the ROTATED value, which can lie a binade above
    max(|a|, |b|): up to 1.41 of this bar in principle.  Measured on these inputs: a few halves per case differ, the worst at 0.63 of the bar.)"""
    k0, v0 = f16_caches(hd)
    f = table(hd)
    kd, vd, fd = DB.from_numpy(k0), DB.from_numpy(v0), DB.from_numpy(f)
    KO.kv_shift(kd, vd, L, S, NKV, hd, src0, dst0, n, inv_freq=fd, theta_base=THETA, interleaved=interleaved)
    k1 = kd.numpy(np.uint16).reshape(k0.shape)
    v1 = vd.numpy(np.uint16).reshape(v0.shape)
    want_k, want_v = KO.shift_f16_ref(k0, v0, src0, dst0, n, hd, inv_freq=f, interleaved=interleaved)
    assert np.array_equal(v1, want_v)                                   # V: moved rows bit for bit, everything else unchanged
    outside = np.ones(S, bool)
    outside[dst0:dst0 + n] = False
    assert np.array_equal(k1[:, outside], k0[:, outside])               # K outside the destination rows: unchanged
    got = k1[:, dst0:dst0 + n].view(np.float16).astype(np.float64)
    want = want_k[:, dst0:dst0 + n].view(np.float16).astype(np.float64)
    bar = 2.0 ** -10 * KO.pair_max(k0[:, src0:src0 + n].view(np.float16), hd, interleaved) + 2.0 ** -24
    err = np.abs(got - want)
    print("f16 hd %d interleaved %d (%d,%d,%d): worst err / bar = %.3f, %d of %d halves differ from the checker" %
          (hd, interleaved, src0, dst0, n, float((err / bar).max()), int((got != want).sum()), got.size))
    assert (err <= bar).all()


def test_kv_shift_f16_without_a_table_uses_the_forward_kernels_frequency():
    """inv_freq = NULL: 1 / (float)pow((double)theta, (double)((2.0f * i) / head_dim)) in the kernel, the checker's default; head_dim 80 too"""
    for hd in (80, 128):
        r = rng(1000 + hd)
        k0 = r.standard_normal((L, S, NKV * hd)).astype(np.float16).view(np.uint16)
        v0 = r.standard_normal((L, S, NKV * hd)).astype(np.float16).view(np.uint16)
        kd, vd = DB.from_numpy(k0), DB.from_numpy(v0)
        KO.kv_shift(kd, vd, L, S, NKV, hd, 20, 5, 70, theta_base=THETA)
        want_k, want_v = KO.shift_f16_ref(k0, v0, 20, 5, 70, hd, theta=THETA)
        assert np.array_equal(vd.numpy(np.uint16).reshape(v0.shape), want_v)
        k1 = kd.numpy(np.uint16).reshape(k0.shape)
        assert np.array_equal(k1[:, :5], k0[:, :5]) and np.array_equal(k1[:, 75:], k0[:, 75:])
        err = np.abs(k1[:, 5:75].view(np.float16).astype(np.float64) - want_k[:, 5:75].view(np.float16).astype(np.float64))
        bar = 2.0 ** -10 * KO.pair_max(k0[:, 20:90].view(np.float16), hd) + 2.0 ** -24
        assert (err <= bar).all()


# ------------------------------------------------------------------------------------------------ Q8
@pytest.mark.parametrize("src0,dst0,n", CASES)
@pytest.mark.parametrize("interleaved", [False, True])
def test_kv_shift_q8_against_the_exact_rotation(interleaved, src0, dst0, n):
    """K: the dequantised rows within 0.625 amax / 127 of the float64 rotation of the dequantised source rows (amax: the rotated block's largest
    magnitude) -- half a quantisation step plus the half-rounded scale's 0.062 of a step, with margin; V blocks bit for bit; every byte of both whole
    buffers (quants, scales, the padding behind a layer) outside the destination rows unchanged."""
    hd = 128
    kb, vb = q8_caches()
    row = NKV * hd
    lb = kv_q8.cache_bytes(S, NKV, hd)
    kraw0, vraw0 = KO.q8_blocks_to_planes(kb, lb), KO.q8_blocks_to_planes(vb, lb)
    kraw0[np.arange(L)[:, None] * lb + np.arange(S * row * 17 // 16, lb)[None, :]] = 0x5A        # the padding behind each layer: a pattern to keep
    f = table(hd)
    kd, vd, fd = DB.from_numpy(kraw0), DB.from_numpy(vraw0), DB.from_numpy(f)
    KO.kv_shift_q8(kd, vd, L, S, NKV, hd, src0, dst0, n, inv_freq=fd, theta_base=THETA, interleaved=interleaved)
    kraw1, vraw1 = kd.numpy(np.uint8), vd.numpy(np.uint8)
    want_kb, want_vb = KO.shift_q8_ref(kb, vb, src0, dst0, n, hd, inv_freq=f, interleaved=interleaved)
    assert np.array_equal(vraw1, KO.q8_blocks_to_planes(want_vb, lb))                            # V: the whole buffer is the checker's
    dest = np.zeros(L * lb, bool)                                                                # the destination rows' bytes: quants and scales
    for l in range(L):
        dest[l * lb + dst0 * row:l * lb + (dst0 + n) * row] = True
        s0 = l * lb + S * row + dst0 * (row // 32) * 2
        dest[s0:s0 + n * (row // 32) * 2] = True
    assert np.array_equal(kraw1[~dest], kraw0[~dest])
    k1 = KO.q8_planes_to_blocks(kraw1, L, S, row)
    exact = KO.rotate_f64(kv_q8.dequantize_exact(kb[:, src0:src0 + n]), dst0 - src0, hd, inv_freq=f, interleaved=interleaved)
    got = kv_q8.dequantize_exact(k1[:, dst0:dst0 + n])
    amax = np.abs(exact.reshape(exact.shape[:-1] + (-1, 32))).max(axis=-1)
    bar = np.repeat(0.625 * amax / 127.0, 32, axis=-1)
    err = np.abs(got - exact)
    same = int((k1[:, dst0:dst0 + n] == want_kb[:, dst0:dst0 + n]).all(axis=-1).sum())
    print("q8 interleaved %d (%d,%d,%d): worst err / bar = %.3f, %d of %d blocks equal the checker's" %
          (interleaved, src0, dst0, n, float((err / bar).max()), same, L * n * (row // 32)))
    assert (err <= bar).all()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_return_their_status_and_leave_the_buffers_unchanged():
    hd = 128
    k0, v0 = f16_caches(hd)
    kd, vd = DB.from_numpy(k0), DB.from_numpy(v0)
    kb, vb = q8_caches()
    lb = kv_q8.cache_bytes(S, NKV, hd)
    kq0, vq0 = KO.q8_blocks_to_planes(kb, lb), KO.q8_blocks_to_planes(vb, lb)
    kq, vq = DB.from_numpy(kq0), DB.from_numpy(vq0)
    bad_rows = [(-1, -2, 4), (8, -1, 4), (8, 8, 4), (8, 9, 4), (8, 4, 0), (8, 4, -3), (8, 4, 89), (96, 4, 1), (200, 100, 4)]
    for src0, dst0, n in bad_rows:
        assert KO.kv_shift_status(kd, vd, L, S, NKV, hd, src0, dst0, n, theta_base=THETA) == NTK_E_SHAPE, (src0, dst0, n)
        assert KO.kv_shift_q8_status(kq, vq, L, S, NKV, hd, src0, dst0, n, theta_base=THETA) == NTK_E_SHAPE, (src0, dst0, n)
    assert KO.kv_shift_status(kd, vd, L, S, NKV, 96, 8, 4, 4, theta_base=THETA) == NTK_E_SHAPE       # a head size the attention kernels do not take
    assert KO.kv_shift_q8_status(kq, vq, L, S, NKV, 64, 8, 4, 4, theta_base=THETA) == NTK_E_SHAPE    # the 8-bit store's limit: head_dim 128 only
    assert KO.kv_shift_status(None, vd, L, S, NKV, hd, 8, 4, 4, theta_base=THETA) == NTK_E_NULL
    assert KO.kv_shift_status(kd, None, L, S, NKV, hd, 8, 4, 4, theta_base=THETA) == NTK_E_NULL
    assert KO.kv_shift_q8_status(None, vq, L, S, NKV, hd, 8, 4, 4, theta_base=THETA) == NTK_E_NULL
    assert KO.kv_shift_q8_status(kq, None, L, S, NKV, hd, 8, 4, 4, theta_base=THETA) == NTK_E_NULL
    assert np.array_equal(kd.numpy(np.uint16).reshape(k0.shape), k0) and np.array_equal(vd.numpy(np.uint16).reshape(v0.shape), v0)
    assert np.array_equal(kq.numpy(np.uint8), kq0) and np.array_equal(vq.numpy(np.uint8), vq0)
