"""ntk_qk_norm on the GPU (csrc/qk_norm.hip): RMSNorm of every head of q [n_rows][n_heads * head_dim] by wq[head_dim] and of k [n_rows][n_kv_heads *
head_dim] by wk[head_dim], in place and in one launch, against O.rmsnorm per head and against a float64 RMSNorm, both at the bar of
tests/test_hip_kernels.py::test_rmsnorm -- 2e-6 x max |ref| + 1e-6 -- taken per head (the head's own maximum: the stricter reading).

Shapes: rows 1 / 2 / 17 x (heads, KV heads) (1, 1) / (4, 2) / (14, 2) / (32, 8) -- two waves, six (a workgroup and a half), sixteen, forty -- x head_dim
64 (one float per lane), 128 (float2), 256 (float4), 80 and 96 (lane-strided, a second partial pass over the lanes), from 256-byte aligned bases and with
every buffer moved by one float (lane-strided throughout: nothing else may be assumed).  q, a v-like buffer and k lie back to back as in the engine's
workspace, poisoned floats in front and behind: the launch writes q and k and nothing else.  Heads differ in magnitude by powers of two from 2^-8 to 2^8.

Run on the MI355X box:  python -m pytest tests/test_qk_norm_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from ntransformer_amd import _lib, ops
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROWS = (1, 2, 17)
HEADS = [(1, 1), (4, 2), (14, 2), (32, 8)]
HEAD_DIMS = [64, 128, 256, 80, 96]
GUARD = 16
POISON = np.float32(-7.25e8)
EPS = 1e-6


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


class Arena:
    """[poison x off][q][v-like][k][poison x GUARD] on the device, `off` floats behind a 256-byte aligned base: the engine's q | k | v neighbourhood"""

    def __init__(self, q, k, off, vlike=None):
        self.off = off
        self.v = np.full(k.size, POISON, np.float32) if vlike is None else vlike.astype(np.float32).reshape(-1)
        self.nq, self.nv, self.nk = q.size, self.v.size, k.size
        self.image = np.concatenate([np.full(off, POISON, np.float32), q.astype(np.float32).reshape(-1), self.v, k.astype(np.float32).reshape(-1),
                                     np.full(GUARD, POISON, np.float32)])
        self.dev = DB.from_numpy(self.image)
        self.q_ptr = self.dev.at(4 * off)
        self.k_ptr = self.dev.at(4 * (off + self.nq + self.nv))

    def read(self):
        """(q, k) after checking that the floats in front, between (the v-like buffer) and behind hold their bits"""
        got = self.dev.numpy(np.float32, self.image.size)
        a, b, c = self.off, self.off + self.nq, self.off + self.nq + self.nv
        assert same_bits(got[:a], self.image[:a]), "wrote in front of q"
        assert same_bits(got[b:c], self.image[b:c]), "wrote between q and k"
        assert same_bits(got[c + self.nk:], self.image[c + self.nk:]), "wrote behind k"
        return got[a:b].copy(), got[c:c + self.nk].copy()


class Vec:
    def __init__(self, host, off):
        self.off, self.n = off, host.size
        self.image = np.concatenate([np.full(off, POISON, np.float32), host.astype(np.float32), np.full(GUARD, POISON, np.float32)])
        self.dev = DB.from_numpy(self.image)
        self.ptr = self.dev.at(4 * off)

    def unchanged(self):
        return same_bits(self.dev.numpy(np.float32, self.image.size), self.image)


def inputs(rows, nh, nkv, hd, seed=0):
    r = np.random.Generator(np.random.Philox(key=[20261022, 100000 * seed + 1000 * rows + 10 * (nh + nkv) + hd]))
    q = (2.0 * r.standard_normal((rows, nh, hd)) * np.exp2(r.integers(-8, 9, (rows, nh, 1)))).astype(np.float32)
    k = (2.0 * r.standard_normal((rows, nkv, hd)) * np.exp2(r.integers(-8, 9, (rows, nkv, 1)))).astype(np.float32)
    wq = (1.0 + 0.5 * r.uniform(-1, 1, hd)).astype(np.float32)
    wk = (1.0 + 0.5 * r.uniform(-1, 1, hd)).astype(np.float32)
    return q, k, wq, wk


def launch(q, k, wq, wk, off, eps=EPS, vlike=None):
    """-> (q', k') of one launch; the weights are read only"""
    rows, nh, hd = q.shape
    nkv = k.shape[1]
    ar, dq, dk = Arena(q, k, off, vlike), Vec(wq, off), Vec(wk, off)
    ops.qk_norm(ar.q_ptr, ar.k_ptr, dq.ptr, dk.ptr, rows, nh, nkv, hd, eps)
    ops.synchronize()
    gq, gk = ar.read()
    assert dq.unchanged() and dk.unchanged()
    return gq.reshape(q.shape), gk.reshape(k.shape)


def rmsnorm64(x, w, eps):
    x = x.astype(np.float64)
    return x / np.sqrt((x * x).mean(axis=-1, keepdims=True) + np.float64(np.float32(eps))) * w.astype(np.float64)


def within_the_bar(got, ref):
    """per head: |got - ref| <= 2e-6 x max |ref over the head| + 1e-6"""
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64)).max(axis=-1)
    bar = 2e-6 * np.abs(ref.astype(np.float64)).max(axis=-1) + 1e-6
    return bool((err <= bar).all()), float((err / bar).max())


# ------------------------------------------------------------------------------------------------ parity
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("hd", HEAD_DIMS)
@pytest.mark.parametrize("heads", HEADS, ids=lambda h: "%dx%d" % h)
def test_qk_norm_matches_the_oracle_and_float64_per_head(heads, hd, off):
    nh, nkv = heads
    for rows in ROWS:
        q, k, wq, wk = inputs(rows, nh, nkv, hd)
        r = np.random.Generator(np.random.Philox(key=[20261022, 9]))
        vlike = r.standard_normal(rows * nkv * hd).astype(np.float32)
        gq, gk = launch(q, k, wq, wk, off, vlike=vlike)
        for got, x, w, what in ((gq, q, wq, "q"), (gk, k, wk, "k")):
            ref = O.rmsnorm(x.reshape(-1, hd), w, EPS).reshape(x.shape)
            ok, worst = within_the_bar(got, ref)
            assert np.isfinite(got).all() and ok, (what, "vs O.rmsnorm", rows, heads, hd, off, worst)
            ok, worst = within_the_bar(got, rmsnorm64(x, w, EPS))
            assert ok, (what, "vs float64", rows, heads, hd, off, worst)


# ------------------------------------------------------------------------------------------------ the same bits
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_the_bits_depend_on_head_dim_and_alignment_alone(hd):
    nh, nkv, rows = 14, 2, 17
    q, k, wq, wk = inputs(rows, nh, nkv, hd, seed=1)
    for off in (0, 1):
        a = launch(q, k, wq, wk, off)
        b = launch(q, k, wq, wk, off)
        assert same_bits(a[0], b[0]) and same_bits(a[1], b[1]), "repeated launches"
        # each row of the 17-row launch = its one-row launch
        for t in (0, 1, 8, 16):
            one = launch(q[t:t + 1], k[t:t + 1], wq, wk, off)
            assert same_bits(one[0][0], a[0][t]) and same_bits(one[1][0], a[1][t]), ("row", t, off)
        # a head's result does not depend on its companions: alone in a (1, 1) launch, as q and as k; and among other heads in another order
        for h in (0, 5, 13):
            solo = launch(q[:, h:h + 1], k[:, :1], wq, wk, off)
            assert same_bits(solo[0][:, 0], a[0][:, h]) and same_bits(solo[1][:, 0], a[1][:, 0]), ("head", h, off)
        rev = launch(q[:, ::-1].copy(), k[:, ::-1].copy(), wq, wk, off)
        assert same_bits(rev[0][:, ::-1], a[0]) and same_bits(rev[1][:, ::-1], a[1])
    al, mv = launch(q, k, wq, wk, 0), launch(q, k, wq, wk, 1)
    if hd in (128, 256):          # 8- / 16-byte accesses from aligned bases, lane-strided elements otherwise: another order of the sum, the same bar
        for g, x, w in ((mv[0], q, wq), (mv[1], k, wk)):
            assert within_the_bar(g, O.rmsnorm(x.reshape(-1, hd), w, EPS).reshape(x.shape))[0]
        assert within_the_bar(mv[0], al[0])[0] and within_the_bar(mv[1], al[1])[0]
    else:                         # lane-strided either way
        assert same_bits(al[0], mv[0]) and same_bits(al[1], mv[1])


def test_mixed_alignment_is_decided_per_buffer():
    """an aligned q (float2 at head_dim 128) beside a k moved by one float and an unaligned wq: each buffer the bits of its own form"""
    rows, nh, nkv, hd = 3, 4, 2, 128
    q, k, wq, wk = inputs(rows, nh, nkv, hd, seed=2)
    al, mv = launch(q, k, wq, wk, 0), launch(q, k, wq, wk, 1)
    vpad = np.full(rows * nkv * hd + 1, POISON, np.float32)          # (one float more between q and k: q aligned, k not)
    ar, dq, dk = Arena(q, k, 0, vlike=vpad), Vec(wq, 0), Vec(wk, 0)
    ops.qk_norm(ar.q_ptr, ar.k_ptr, dq.ptr, dk.ptr, rows, nh, nkv, hd, EPS)
    ops.synchronize()
    gq, gk = ar.read()
    assert same_bits(gq.reshape(q.shape), al[0]) and same_bits(gk.reshape(k.shape), mv[1])
    ar, dq, dk = Arena(q, k, 0), Vec(wq, 1), Vec(wk, 0)                  # an unaligned weight vector makes its buffer lane-strided
    ops.qk_norm(ar.q_ptr, ar.k_ptr, dq.ptr, dk.ptr, rows, nh, nkv, hd, EPS)
    ops.synchronize()
    gq, gk = ar.read()
    assert same_bits(gq.reshape(q.shape), mv[0]) and same_bits(gk.reshape(k.shape), al[1])


# ------------------------------------------------------------------------------------------------ edge rows
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("hd", HEAD_DIMS)
def test_zero_nan_and_overflowing_heads(hd, off):
    rows, nh, nkv = 2, 4, 2
    q, k, wq, wk = inputs(rows, nh, nkv, hd, seed=3)
    q[0, 1] = 0.0                    # an all-zero head: zeros, not NaN (1 / sqrt(eps) is finite)
    k[1, 0] = 0.0
    q[1, 2, hd // 3] = np.nan        # a NaN stays in its head
    q[0, 3] = np.float32(1e19) * np.sign(q[0, 3])          # the sum of squares overflows: what O.rmsnorm gives
    k[0, 1] = np.float32(1e19)
    gq, gk = launch(q, k, wq, wk, off)
    assert not np.any(gq[0, 1]) and not np.any(gk[1, 0])
    assert np.isnan(gq[1, 2]).all()
    finite = np.ones((rows, nh), bool)
    finite[1, 2] = False
    assert np.isfinite(gq[finite]).all() and np.isfinite(gk).all()
    with np.errstate(all="ignore"):
        rq = O.rmsnorm(q.reshape(-1, hd), wq, EPS).reshape(q.shape)
        rk = O.rmsnorm(k.reshape(-1, hd), wk, EPS).reshape(k.shape)
    assert same_bits(gq[0, 3], rq[0, 3]) and same_bits(gk[0, 1], rk[0, 1])          # (zeros: 1 / sqrt(inf) = 0)
    assert within_the_bar(gq[finite], rq[finite])[0] and within_the_bar(gk, rk)[0]


def test_wq_and_wk_are_each_honoured():
    rows, nh, nkv, hd = 2, 4, 2, 128
    q, k, wq, wk = inputs(rows, nh, nkv, hd, seed=4)
    own, swapped = launch(q, k, wq, wk, 0), launch(q, k, wk, wq, 0)
    assert within_the_bar(own[0], O.rmsnorm(q.reshape(-1, hd), wq, EPS).reshape(q.shape))[0]
    assert within_the_bar(swapped[0], O.rmsnorm(q.reshape(-1, hd), wk, EPS).reshape(q.shape))[0]
    assert within_the_bar(swapped[1], O.rmsnorm(k.reshape(-1, hd), wq, EPS).reshape(k.shape))[0]
    assert np.abs(own[0] - swapped[0]).max() > 0.05 and np.abs(own[1] - swapped[1]).max() > 0.05
    # eps is honoured too: a tiny head is held down by a large eps
    small = (q * np.float32(1e-3)).astype(np.float32)
    big_eps = launch(small, k, wq, wk, 0, eps=1.0)
    assert within_the_bar(big_eps[0], O.rmsnorm(small.reshape(-1, hd), wq, 1.0).reshape(q.shape))[0]


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_poisoned_buffers_unchanged():
    L = _lib.lib()
    rows, nh, nkv, hd = 4, 4, 2, 64
    poison_q, poison_k = np.full((rows, nh, hd), POISON, np.float32), np.full((rows, nkv, hd), POISON, np.float32)
    ar = Arena(poison_q, poison_k, 0)
    wq, wk = Vec(np.ones(hd, np.float32), 0), Vec(np.ones(hd, np.float32), 0)
    call = lambda q, k, a, b, n, h, kv, d: L.ntk_qk_norm(q, k, a, b, n, h, kv, d, EPS, None)
    good = (ar.q_ptr, ar.k_ptr, wq.ptr, wk.ptr)
    for i in range(4):                                                    # NTK_E_NULL: any NULL pointer
        ptrs = list(good)
        ptrs[i] = None
        assert call(*ptrs, rows, nh, nkv, hd) == -5, i
    assert call(None, None, None, None, rows, nh, nkv, hd) == -5
    assert call(*good, rows, nh, nkv, 0) == -2                            # NTK_E_SHAPE: head_dim <= 0 ...
    assert call(*good, rows, nh, nkv, -64) == -2
    assert call(*good, rows, nh, nkv, 63) == -2                           # ... or odd
    assert call(*good, rows, 0, nkv, hd) == -2                            # n_heads <= 0
    assert call(*good, rows, -4, nkv, hd) == -2
    assert call(*good, rows, nh, 0, hd) == -2                             # n_kv_heads <= 0
    assert call(*good, rows, nh, -2, hd) == -2
    assert call(*good, -1, nh, nkv, hd) == -2                             # n_rows < 0
    assert call(*good, 0, nh, nkv, hd) == 0                               # no rows: NTK_OK, nothing launched
    ops.synchronize()
    gq, gk = ar.read()
    assert same_bits(gq, poison_q.reshape(-1)) and same_bits(gk, poison_k.reshape(-1)) and wq.unchanged() and wk.unchanged()
    with pytest.raises(_lib.NtkError) as ei:
        ops.qk_norm(*good, rows, nh, nkv, 63, EPS)
    assert ei.value.status == -2
    assert call(*good, rows, nh, nkv, hd) == 0                            # (and the good call does write)
    ops.synchronize()
    gq, gk = ar.read()
    assert not same_bits(gq, poison_q.reshape(-1)) and not same_bits(gk, poison_k.reshape(-1))
