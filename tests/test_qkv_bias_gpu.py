"""ntk_qkv_bias on the GPU (csrc/qkv_bias.hip): q [n_rows][q_dim] += bq, k / v [n_rows][kv_dim] += bk / bv in one launch, against numpy's float32 addition
BIT FOR BIT -- every element is one F32 add.

Shapes: one row of the smallest vector width (8, 8); a decode step of Qwen2.5-7B (1, 3584, 512); a few rows of the tiny models (3, 256, 128); rows of
Qwen2.5-0.5B's widths beyond one workgroup (17, 896, 128); (70, 258, 2): a width that is no multiple of 4, so rows start off 16-byte alignment and the
launch walks it element by element; and a 1024-token prompt of the 7B shape (1024, 3584, 512).  Every shape runs from 256-byte aligned bases (the 16-byte
pieces where the dimension allows them) and with every buffer moved by one float (scalar accesses throughout: nothing else may be assumed).  Every buffer
is followed by 16 guard floats, which the launch must leave alone; values mix magnitudes from 2^-20 to 2^20 and both signs.

Run on the MI355X box:  python -m pytest tests/test_qkv_bias_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from ntransformer_amd import _lib, ops
from ntransformer_amd.ops import DeviceBuffer as DB

pytestmark = pytest.mark.gpu
SHAPES = [(1, 8, 8), (1, 3584, 512), (3, 256, 128), (17, 896, 128), (70, 258, 2), (1024, 3584, 512)]
GUARD = 16
POISON = np.float32(-7.25e8)


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def values(r, n):
    return (r.standard_normal(n) * np.exp2(r.integers(-20, 21, n))).astype(np.float32)


class Buf:
    """`n` floats on the device, `off` floats behind a 256-byte aligned base, GUARD poisoned floats in front (where off > 0) and behind"""

    def __init__(self, host, off):
        self.n, self.off = host.size, off
        self.image = np.concatenate([np.full(off, POISON, np.float32), host.astype(np.float32), np.full(GUARD, POISON, np.float32)])
        self.dev = DB.from_numpy(self.image)
        self.ptr = self.dev.at(4 * off)

    def read(self):
        got = self.dev.numpy(np.float32, self.image.size)
        assert np.array_equal(got[:self.off].view(np.uint32), self.image[:self.off].view(np.uint32)), "wrote in front of the buffer"
        assert np.array_equal(got[self.off + self.n:].view(np.uint32), self.image[self.off + self.n:].view(np.uint32)), "wrote behind the buffer"
        return got[self.off:self.off + self.n]


def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def run_case(n_rows, q_dim, kv_dim, off, missing=None, seed=0):
    r = np.random.Generator(np.random.Philox(key=[20261021, 1000 * seed + n_rows + q_dim]))
    x = {w: values(r, n_rows * d).reshape(n_rows, d) for w, d in (("q", q_dim), ("k", kv_dim), ("v", kv_dim))}
    b = {w: values(r, d) for w, d in (("q", q_dim), ("k", kv_dim), ("v", kv_dim))}
    dx = {w: Buf(x[w].reshape(-1), off) for w in "qkv"}
    db = {w: Buf(b[w], off) for w in "qkv"}
    ops.qkv_bias(dx["q"].ptr, dx["k"].ptr, dx["v"].ptr, *[None if w == missing else db[w].ptr for w in "qkv"], n_rows, q_dim, kv_dim)
    ops.synchronize()
    for w in "qkv":
        want = x[w] if w == missing else x[w] + b[w][None, :]              # numpy float32 addition
        assert want.dtype == np.float32
        assert same_bits(dx[w].read().reshape(x[w].shape), want), (w, n_rows, q_dim, kv_dim, off, missing)
        assert same_bits(db[w].read(), b[w])                                # (the biases are read only)


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_qkv_bias_is_numpy_float32_addition_bit_for_bit(shape, off):
    run_case(*shape, off)


@pytest.mark.parametrize("missing", ["q", "k", "v"])
@pytest.mark.parametrize("shape", [(1, 3584, 512), (3, 256, 128), (70, 258, 2)], ids=lambda s: "x".join(map(str, s)))
def test_a_missing_bias_leaves_its_buffer_untouched(shape, missing):
    for off in (0, 1):
        run_case(*shape, off, missing=missing, seed=1)


def test_two_missing_biases_and_mixed_alignment():
    """only one bias present (its buffer alone is written); an aligned q beside k and v moved by one float (the choice of width is per buffer)"""
    r = np.random.Generator(np.random.Philox(key=[20261021, 77]))
    n_rows, q_dim, kv_dim = 5, 256, 128
    for present in "qkv":
        x = {w: values(r, n_rows * (q_dim if w == "q" else kv_dim)) for w in "qkv"}
        b = values(r, q_dim if present == "q" else kv_dim)
        dx = {w: Buf(x[w], 0 if w == "q" else 1) for w in "qkv"}
        dbias = Buf(b, 1 if present == "q" else 0)
        ops.qkv_bias(dx["q"].ptr, dx["k"].ptr, dx["v"].ptr, *[dbias.ptr if w == present else None for w in "qkv"], n_rows, q_dim, kv_dim)
        ops.synchronize()
        for w in "qkv":
            want = x[w].reshape(n_rows, -1) + b[None, :] if w == present else x[w].reshape(n_rows, -1)
            assert same_bits(dx[w].read(), want.reshape(-1)), (present, w)


def test_refusals_launch_nothing():
    L = _lib.lib()
    r = np.random.Generator(np.random.Philox(key=[20261021, 78]))
    x = {w: Buf(values(r, 4 * 64), 0) for w in "qkv"}
    b = {w: Buf(values(r, 64), 0) for w in "qkv"}
    before = {w: x[w].read().copy() for w in "qkv"}
    call = lambda q, k, v, bq, bk, bv, n, qd, kd: L.ntk_qkv_bias(q, k, v, bq, bk, bv, n, qd, kd, None)
    ptr = lambda d: [d[w].ptr for w in "qkv"]
    assert call(*ptr(x), *ptr(b), -1, 64, 64) == -2                       # NTK_E_SHAPE: negative rows
    assert call(*ptr(x), *ptr(b), 4, 0, 64) == -2                         # ... a dimension <= 0
    assert call(*ptr(x), *ptr(b), 4, 64, -64) == -2
    assert call(None, x["k"].ptr, x["v"].ptr, *ptr(b), 4, 64, 64) == -5   # NTK_E_NULL: a bias without its buffer
    assert call(x["q"].ptr, None, x["v"].ptr, *ptr(b), 4, 64, 64) == -5
    assert call(x["q"].ptr, x["k"].ptr, None, *ptr(b), 4, 64, 64) == -5
    assert call(*ptr(x), *ptr(b), 0, 64, 64) == 0                         # no rows: NTK_OK, nothing launched
    assert call(*ptr(x), None, None, None, 4, 64, 64) == 0                # no bias at all: NTK_OK, nothing launched
    assert call(None, None, None, None, None, None, 4, 64, 64) == 0
    ops.synchronize()
    for w in "qkv":
        assert same_bits(x[w].read(), before[w]), w
    with pytest.raises(_lib.NtkError) as ei:
        ops.qkv_bias(*ptr(x), *ptr(b), 4, 64, 0)
    assert ei.value.status == -2
    assert call(x["q"].ptr, None, None, b["q"].ptr, None, None, 4, 64, 64) == 0      # (a buffer without a bias need not exist)
    ops.synchronize()
    assert not same_bits(x["q"].read(), before["q"]) and same_bits(x["k"].read(), before["k"])
