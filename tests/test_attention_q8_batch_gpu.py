"""ntk_attention_decode_q8_batch (csrc/attention_q8.hip, attention_q8_decode.hip.h): decode attention over the 8-bit (Q8_0) KV cache for up to 16
sequences, each with its own pair of caches and its own position, in one launch + one combine launch -- through the C ABI.  Every row against
 (1) ntk_attention_decode_q8 on a copy of that row's caches at the same split count: output and WHOLE caches bit-identical (one device function,
     one split count: the bar is equality);
 (2) a float64 attention over the exactly dequantised cache, the stored new row included, at test_kv_q8_gpu.check_decode's bars: output 3e-5, stored V
     blocks bit-exact against the numpy quantiser, stored K quants within one step / scales within 2^-10 of the numpy quantiser of the oracle's rotation;
 (3) what it must NOT touch: every byte of every row's caches outside the written row, the junk tail included.
Rows from each position on hold NaN / inf scale patterns and 0x80 quants before the launch (run_decode(junk=True) of test_kv_q8_gpu.py).

Run on the MI355X box:  python -m pytest tests/test_attention_q8_batch_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from ntransformer_amd import kv_q8, ops
from ntransformer_amd.kv_q8 import Q8Cache
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O

pytestmark = pytest.mark.gpu

THETA = 500000.0
HD = 128
GEOMETRIES = [(8, 2), (16, 2), (16, 1), (3, 3)]   # 4, 8, 16 and 1 query heads per KV head
# the position lists of tests/test_attention_batch_gpu.py: 0, 1, 15 / 16, 31 / 32 / 33, 543 / 544, 4095 and repeats mixed inside one batch
POSITIONS = {1: [543], 2: [0, 4095], 3: [33, 0, 2047], 16: [0, 1, 15, 16, 31, 32, 33, 543, 544, 1023, 2047, 4095, 0, 32, 544, 1]}
SPLITS = [1, 3, 4, 16, 32]                        # 3: more splits than some rows have chunks; 4 / 16 / 32: the engine's three regimes
JUNK = np.array([0x7E00, 0xFE00, 0x7C00, 0xFC00, 0x7BFF, 0xFFFF], np.uint16)   # NaN / inf / 65504 scale patterns

_pool = {}


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def _blocks(n, nb, salt):
    """n rows of nb canonical blocks with unit-variance values (test_kv_q8_gpu.random_blocks: quants uniform in [-127, 127], scales uniform in
    [0.5, 1.4] / 73.3), windows (by `salt`) of pools drawn once"""
    if "q" not in _pool:
        r = np.random.Generator(np.random.Philox(key=[20261019, 1]))
        _pool["q"] = r.integers(-127, 128, 1 << 22).astype(np.int8)
        _pool["d"] = (r.uniform(0.5, 1.4, 1 << 18) / 73.3).astype(np.float16)
    q, d = _pool["q"], _pool["d"]
    qo, do = (salt * 104729) % (q.size - 1), (salt * 7919) % (d.size - 1)
    return kv_q8.to_blocks(np.resize(np.roll(d, -do), n * nb).reshape(n, nb), np.resize(np.roll(q, -qo), n * nb * 32).reshape(n, nb, 32))


def _inv_freq():   # the engine's host-computed table: 1 / powf(theta, 2i / hd) in float32
    i = np.arange(HD // 2, dtype=np.float32)
    return (np.float32(1.0) / np.power(np.float32(THETA), (np.float32(2.0) * i) / np.float32(HD))).astype(np.float32)


def _case(positions, nh, nkv, max_seq, seed):
    """q, k, v [B][..] and per row the canonical blocks of rows [0, pos) and the RAW device image of its (K, V) caches: those rows, then junk"""
    B, nb = len(positions), nkv * HD // 32
    r = np.random.Generator(np.random.Philox(key=[20261019, seed]))
    q = r.standard_normal((B, nh * HD)).astype(np.float32)
    k = r.standard_normal((B, nkv * HD)).astype(np.float32)
    v = r.standard_normal((B, nkv * HD)).astype(np.float32)
    blocks, raws = [], []
    for b, pos in enumerate(positions):
        pair, raw = [], []
        for side in range(2):
            c = Q8Cache(max_seq, nkv, HD)
            jd = JUNK[r.integers(0, len(JUNK), (max_seq - pos, nb))].view(np.float16)
            c.write_blocks(pos, kv_q8.to_blocks(jd, np.full((max_seq - pos, nb, 32), -128, np.int8)))
            blk = _blocks(pos, nb, seed + 2 * b + side)
            if pos:
                c.write_blocks(0, blk)
            pair.append(blk)
            raw.append(c.raw().copy())
        blocks.append(tuple(pair))
        raws.append(tuple(raw))
    return q, k, v, blocks, raws


def _caches(raws, nkv, max_seq):
    """fresh device caches holding the raw images"""
    out = []
    for kr, vr in raws:
        kc, vc = Q8Cache(max_seq, nkv, HD), Q8Cache(max_seq, nkv, HD)
        kc.buf.upload(kr, 0); vc.buf.upload(vr, 0)
        out.append((kc, vc))
    return out


def _run_batch(q, k, v, raws, positions, nh, nkv, max_seq, nsplit, table, order=None):
    """the batched launch over rows `order` (default: as given); returns out [B][nh * HD] and the caches (device), in the launch's row order"""
    B = len(positions)
    order = list(range(B)) if order is None else order
    caches = _caches([raws[b] for b in order], nkv, max_seq)
    od = DB.from_numpy(np.full(B * nh * HD, np.nan, np.float32))
    inv = DB.from_numpy(_inv_freq()) if table else None
    kv_q8.attention_decode_q8_batch(od, DB.from_numpy(q[order]), DB.from_numpy(k[order]), DB.from_numpy(v[order]), caches,
                                    DB.from_numpy(np.array([positions[b] for b in order], np.int32)), B, nh, nkv, HD, max_seq,
                                    float(1 / np.sqrt(HD)), THETA, nsplit, inv_freq=inv)
    return od.numpy().reshape(B, nh * HD), caches


def _slack(B, nsplit, nh):
    """rows behind the largest position: none where nsplit == 4 (one case per B and geometry with a row ON the last cache row), else a different count per case"""
    return 0 if nsplit == 4 else 1 + (7 * B + nsplit + nh) % 61


@pytest.mark.parametrize("nsplit", SPLITS)
@pytest.mark.parametrize("B", [1, 2, 3, 16])
@pytest.mark.parametrize("nh,nkv", GEOMETRIES)
def test_rows_equal_the_single_row_launch_and_the_float64_reference(nh, nkv, B, nsplit):
    positions = POSITIONS[B]
    max_seq = max(positions) + 1 + _slack(B, nsplit, nh)
    scale = float(1 / np.sqrt(HD))
    table = B % 2 == 0
    per, nb = nkv * HD, nkv * HD // 32
    q, k, v, blocks, raws = _case(positions, nh, nkv, max_seq, 1000 * nh + 10 * B + nsplit)
    out, caches = _run_batch(q, k, v, raws, positions, nh, nkv, max_seq, nsplit, table)
    assert np.isfinite(out).all()
    inv = DB.from_numpy(_inv_freq()) if table else None
    worst = 0.0
    for b, pos in enumerate(positions):
        kc, vc = caches[b]
        got = (kc.raw(), vc.raw())
        # (1) the single-row launch on a copy of this row's caches, the same split count: the same bits, output and whole caches
        (kc1, vc1), = _caches([raws[b]], nkv, max_seq)
        od = DB.from_numpy(np.full(nh * HD, np.nan, np.float32))
        kv_q8.attention_decode_q8(od, DB.from_numpy(q[b]), DB.from_numpy(k[b]), DB.from_numpy(v[b]), kc1, vc1, DB.from_numpy(np.array([pos], np.int32)),
                                  nh, nkv, HD, max_seq, scale, THETA, nsplit, inv_freq=inv)
        assert np.array_equal(out[b], od.numpy()), (b, pos)
        assert np.array_equal(got[0], kc1.raw()) and np.array_equal(got[1], vc1.raw()), (b, pos)
        # (2) the new row against the numpy quantiser, the output against float64 over the exactly dequantised cache (check_decode's bars)
        new_k, new_v = kc.read_blocks(pos, 1), vc.read_blocks(pos, 1)
        rq, rk = O.rope(q[b], k[b], [pos], nh, nkv, HD, THETA)
        assert np.array_equal(new_v, kv_q8.to_blocks(*kv_q8.quantize_q8_0(v[b][None, :]))), (b, pos)
        wd, wq = kv_q8.quantize_q8_0(rk[None, :])
        gd, gq = kv_q8.from_blocks(new_k)
        assert np.abs(gq.astype(np.int32) - wq.astype(np.int32)).max() <= 1, (b, pos)
        assert np.abs(gd.astype(np.float32) - wd.astype(np.float32)).max() <= 2.0 ** -10 * float(wd.max()), (b, pos)
        K = np.concatenate([kv_q8.dequantize_exact(blocks[b][0]), kv_q8.dequantize_exact(new_k)]).reshape(pos + 1, per)
        V = np.concatenate([kv_q8.dequantize_exact(blocks[b][1]), kv_q8.dequantize_exact(new_v)]).reshape(pos + 1, per)
        ref = kv_q8.attention_f64(rq, K, V, nh, nkv, HD, scale)
        err = float(np.abs(out[b] - ref).max())
        worst = max(worst, err)
        assert err <= 3e-5, (b, pos, err)
        # (3) every byte outside the written row keeps its value: earlier rows, the junk tail, the padding
        keep = np.ones(got[0].size, bool)
        keep[pos * per:(pos + 1) * per] = False
        s0 = max_seq * per + pos * nb * 2
        keep[s0:s0 + nb * 2] = False
        for side in range(2):
            assert np.array_equal(got[side][keep], raws[b][side][keep]), (b, pos, side)
    print("nh %d nkv %d B %d nsplit %d max_seq %d: worst |out - f64| = %.3g" % (nh, nkv, B, nsplit, max_seq, worst))


@pytest.mark.parametrize("nh,nkv,B,nsplit", [(nh, nkv, B, ns) for nh, nkv, B in [(16, 2, 16), (8, 2, 3), (3, 3, 16)] for ns in (1, 4, 32)])
def test_permuting_the_rows_permutes_outputs_and_caches(nh, nkv, B, nsplit):
    """A row's result depends on nothing but that row: the same rows in another order (other companions, other entries of the pointer table, other
    slices of the scratch) give the same output bits and the same cache bytes."""
    positions = [min(p, 1023) for p in POSITIONS[B]]
    max_seq = 1024 + 5 * nsplit
    q, k, v, _, raws = _case(positions, nh, nkv, max_seq, 77 + nh + nsplit)
    order = [(5 * i + 3) % B for i in range(B)] if B == 16 else [2, 0, 1]
    assert sorted(order) == list(range(B))
    out_a, c_a = _run_batch(q, k, v, raws, positions, nh, nkv, max_seq, nsplit, True)
    out_b, c_b = _run_batch(q, k, v, raws, positions, nh, nkv, max_seq, nsplit, True, order)
    for i, b in enumerate(order):
        assert np.array_equal(out_b[i], out_a[b]), (i, b)
        assert np.array_equal(c_b[i][0].raw(), c_a[b][0].raw()) and np.array_equal(c_b[i][1].raw(), c_a[b][1].raw()), (i, b)
    assert any(not np.array_equal(c_a[b][0].raw(), raws[b][0]) for b in range(B))   # (the launch did write)


def test_refusals():
    """n_rows 0 and 17, head_dim 64, 17 query heads per KV head (NTK_E_SHAPE); a NULL cache among the first n_rows, a NULL table, NULL scratch
    (NTK_E_NULL): nothing is launched"""
    nh, nkv, max_seq = 8, 2, 64
    z = lambda n: DB.zeros(n * 4)
    pos = DB.from_numpy(np.zeros(32, np.int32))
    mk = lambda n, kvh=nkv, hd=HD: [(Q8Cache(max_seq, kvh, hd), Q8Cache(max_seq, kvh, hd)) for _ in range(n)]

    def call(B, caches, n_heads=nh, n_kv=nkv, hd=HD, **kw):
        return kv_q8.attention_decode_q8_batch_status(z(17 * n_heads * hd), z(17 * n_heads * hd), z(17 * n_kv * hd), z(17 * n_kv * hd), caches, pos, B,
                                                      n_heads, n_kv, hd, max_seq, 0.1, THETA, 4, **kw)

    caches = mk(16)
    assert call(2, caches[:2]) == 0                     # (the same call, accepted)
    assert call(0, caches) == -2 and call(17, caches) == -2
    assert call(2, mk(2, hd=64), hd=64) == -2
    assert call(2, caches[:2], n_heads=34) == -2        # 17 query heads per KV head
    assert call(2, [caches[0], None]) == -5             # NTK_E_NULL
    assert call(2, [caches[0], (caches[1][0], None)]) == -5
    assert call(2, caches[:2], table=False) == -5
    assert call(2, caches[:2], scratch=False) == -5
    assert call(1, [caches[0], None]) == 0              # (an entry past n_rows is not looked at)
