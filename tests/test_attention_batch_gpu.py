"""ntk_attention_decode_batch (csrc/attention_batch.hip): decode attention for up to 16 sequences, each with its own KV cache and position, in
one launch -- through the C ABI, row by row against the oracle's rope + copy_to_kv_cache + attention_decode, against the single-row launch of
the same form, and for what it must NOT touch.  Bars: those of test_hip_kernels.py's single-row tests (named at each assertion).

Every cache row from a row's position on (the position's own row included: the launch writes it) is filled with NaN / inf / junk halves before
the launch, in every case: a result within the bar is then also the proof that nothing past a position entered it."""
import numpy as np
import pytest

from ntransformer_amd import _lib, ops
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O

pytestmark = pytest.mark.gpu

THETA = 500000.0
GEOMETRIES = [(32, 8, 128), (64, 8, 128), (4, 2, 64), (6, 3, 80), (8, 2, 256)]
# per batch size: positions mixed inside one batch; B >= 2 always has position 0 beside the batch's largest
POSITIONS = {1: [543], 2: [0, 4095], 3: [33, 0, 2047], 16: [0, 1, 15, 16, 31, 32, 33, 543, 544, 1023, 2047, 4095, 0, 32, 544, 1]}
JUNK = np.array([0x7E00, 0xFE00, 0x7C00, 0xFC00, 0x7BFF, 0xFBFF, 0x0001, 0x8000], np.uint16)   # NaN, -NaN, +-inf, +-65504, denormal, -0

_pool = {}


def _halves(n, salt):
    """n pseudo-random halves ~ N(0, 1), a window (by `salt`) of one pool drawn once: 16 caches of 4096 rows cost no 16 draws"""
    if "h" not in _pool:
        r = np.random.default_rng(20240607)
        _pool["h"] = r.standard_normal(1 << 22).astype(np.float16).view(np.uint16)
        _pool["j"] = JUNK[r.integers(0, len(JUNK), 1 << 22)]
    h = _pool["h"]
    off = (salt * 104729) % (h.size - 1)
    return np.resize(np.roll(h, -off), n) if n > h.size else np.roll(h, -off)[:n]


def _junk(n, salt):
    _halves(1, 0)
    j = _pool["j"]
    off = (salt * 7919) % (j.size - 1)
    return np.resize(np.roll(j, -off), n)


def _inv_freq(hd):   # the engine's host-computed table: 1/powf(theta, 2i/hd) in float32 (reference rotary.cu:47)
    i = np.arange(hd // 2, dtype=np.float32)
    return (np.float32(1.0) / np.power(np.float32(THETA), (np.float32(2.0) * i) / np.float32(hd))).astype(np.float32)


def _case(positions, nh, nkv, hd, max_seq, seed):
    """inputs of one batch: q, k, v and per row a separately allocated (K, V) cache image with rows [0, pos) random, the rest junk"""
    B = len(positions)
    r = np.random.default_rng(seed)
    q = r.standard_normal((B, nh * hd)).astype(np.float32)
    k = r.standard_normal((B, nkv * hd)).astype(np.float32)
    v = r.standard_normal((B, nkv * hd)).astype(np.float32)
    row = nkv * hd
    caches = []
    for b, pos in enumerate(positions):
        kc, vc = _junk(max_seq * row, seed + 2 * b).copy(), _junk(max_seq * row, seed + 2 * b + 1).copy()
        kc[: pos * row] = _halves(pos * row, seed + 2 * b)
        vc[: pos * row] = _halves(pos * row, seed + 2 * b + 1)
        caches.append((kc, vc))
    return q, k, v, caches


def _run_batch(q, k, v, caches, positions, nh, nkv, hd, max_seq, nsplit, table, order=None):
    """the batched launch over rows `order` (default: as given); returns out [B][nh * hd] and the caches read back, in the given row order"""
    B = len(positions)
    order = list(range(B)) if order is None else order
    kcd = [DB.from_numpy(caches[b][0]) for b in order]
    vcd = [DB.from_numpy(caches[b][1]) for b in order]
    od = DB.from_numpy(np.full(B * nh * hd, np.nan, np.float32))
    inv = DB.from_numpy(_inv_freq(hd)) if table else None
    ops.attention_decode_batch(od, DB.from_numpy(q[order]), DB.from_numpy(k[order]), DB.from_numpy(v[order]), kcd, vcd,
                               DB.from_numpy(np.array([positions[b] for b in order], np.int32)), B, nh, nkv, hd, max_seq,
                               float(1 / np.sqrt(hd)), THETA, nsplit=nsplit, inv_freq=inv)
    out = od.numpy().reshape(B, nh * hd)
    back = [(kd.numpy(np.uint16), vd.numpy(np.uint16)) for kd, vd in zip(kcd, vcd)]
    return out, back


@pytest.mark.parametrize("nsplit", [1, 8, 32, 3])
@pytest.mark.parametrize("B", [1, 2, 3, 16])
@pytest.mark.parametrize("nh,nkv,hd", GEOMETRIES)
def test_attention_decode_batch_rows_equal_the_oracle_and_the_single_row_launch(nh, nkv, hd, B, nsplit):
    """Each row against the oracle's three launches on that row's own cache (output 3e-5, stored V bit-exact, stored K 2e-3 * max(1, |K|max):
    test_attention_decode_fused_equals_rope_store_attend) and against the single-row launch of the same form and split count (output 2e-6,
    cache rows identical: test_attention_decode_split_equals_oracle_and_single_pass); every cache element outside the B written rows keeps
    its bit pattern -- whole caches, other rows' caches and the junk past each position included.  nsplit 32 at (32 | 64, 8, 128): the
    matrix-core form; nsplit 3: more splits than some rows have positions; head_dim 80 splits as little as the single-row kernel does."""
    positions = POSITIONS[B]
    max_seq = max(positions) + 1 + (7 * B + nsplit + nh) % 61          # a different slack per case
    scale = float(1 / np.sqrt(hd))
    table = B % 2 == 0
    seed = 1000 * nh + 10 * B + nsplit
    q, k, v, caches = _case(positions, nh, nkv, hd, max_seq, seed)
    if hd == 80 and nsplit > 1:   # the split kernels take head_dim 64 / 128 / 256
        with pytest.raises(_lib.NtkError):
            _run_batch(q, k, v, caches, positions, nh, nkv, hd, max_seq, nsplit, table)
        return
    out, back = _run_batch(q, k, v, caches, positions, nh, nkv, hd, max_seq, nsplit, table)
    assert np.isfinite(out).all()
    row = nkv * hd
    inv = DB.from_numpy(_inv_freq(hd)) if table else None
    for b, pos in enumerate(positions):
        kc, vc = caches[b]
        # the oracle: rope, store, attend over rows 0 .. pos of this row's cache
        rq, rk = O.rope(q[b], k[b], [pos], nh, nkv, hd, THETA)
        kc_ref, vc_ref = kc.copy(), vc.copy()
        O.copy_to_kv_cache(kc_ref, vc_ref, rk, v[b], 1, nkv, hd, pos, max_seq)
        ref = O.attention_decode(rq, kc_ref, vc_ref, pos + 1, nh, nkv, hd, max_seq, scale)
        err = float(np.abs(out[b] - ref).max())
        assert err <= 3e-5, (b, pos, err)
        got_k, got_v = back[b]
        new = slice(pos * row, (pos + 1) * row)
        assert np.array_equal(got_v[new], vc_ref[new]), (b, pos)
        gk = got_k[new].view(np.float16).astype(np.float32)
        wk = kc_ref[new].view(np.float16).astype(np.float32)
        assert np.abs(gk - wk).max() <= 2e-3 * max(1.0, float(np.abs(wk).max())), (b, pos)
        # nothing else is touched: the whole cache but the written row, bit pattern by bit pattern
        for got, was in ((got_k, kc), (got_v, vc)):
            assert np.array_equal(got[: pos * row], was[: pos * row]), (b, pos)
            assert np.array_equal(got[(pos + 1) * row:], was[(pos + 1) * row:]), (b, pos)
        # the single-row launch of the same form
        kcd, vcd = DB.from_numpy(kc), DB.from_numpy(vc)
        od = DB.from_numpy(np.full(nh * hd, np.nan, np.float32))
        args = (od, DB.from_numpy(q[b]), DB.from_numpy(k[b]), DB.from_numpy(v[b]), kcd, vcd, DB.from_numpy(np.array([pos], np.int32)),
                nh, nkv, hd, max_seq, scale, THETA)
        if nsplit == 1: ops.attention_decode_fused(*args, inv_freq=inv)
        else: ops.attention_decode_split(*args, nsplit, inv_freq=inv)
        assert np.abs(out[b] - od.numpy()).max() <= 2e-6, (b, pos)
        assert np.array_equal(kcd.numpy(np.uint16), got_k) and np.array_equal(vcd.numpy(np.uint16), got_v), (b, pos)


@pytest.mark.parametrize("nh,nkv,hd,B,nsplit", [(nh, nkv, hd, B, ns) for nh, nkv, hd, B in [(32, 8, 128, 16), (32, 8, 128, 3), (4, 2, 64, 16), (8, 2, 256, 16)]
                                                for ns in (1, 8, 32, 3)] + [(6, 3, 80, 3, 1)])   # (head_dim 80 does not split)
def test_attention_decode_batch_permuting_the_rows_permutes_the_results(nh, nkv, hd, B, nsplit):
    """A row's result depends on nothing but that row: the same rows in another order (other companions on every side, other slots of the
    pointer table) give the same output bits and the same cache bytes."""
    positions = [min(p, 1023) for p in POSITIONS[B]]
    max_seq = 1024 + 5 * nsplit
    q, k, v, caches = _case(positions, nh, nkv, hd, max_seq, 77 + nh + nsplit)
    order = [(5 * i + 3) % B for i in range(B)] if B == 16 else [2, 0, 1]
    assert sorted(order) == list(range(B))
    out_a, back_a = _run_batch(q, k, v, caches, positions, nh, nkv, hd, max_seq, nsplit, True)
    out_b, back_b = _run_batch(q, k, v, caches, positions, nh, nkv, hd, max_seq, nsplit, True, order)
    for i, b in enumerate(order):
        assert np.array_equal(out_b[i], out_a[b]), (i, b)
        assert np.array_equal(back_b[i][0], back_a[b][0]) and np.array_equal(back_b[i][1], back_a[b][1]), (i, b)


def test_attention_decode_batch_refusals():
    """B = 0 and B = 17 (NTK_E_SHAPE), a null cache table, a null cache pointer inside it and null positions (NTK_E_NULL): nothing is launched."""
    nh, nkv, hd, max_seq = 4, 2, 64, 64
    mk = lambda n: [DB.zeros(max_seq * nkv * hd * 2) for _ in range(n)]
    z = lambda n: DB.zeros(n * 4)
    common = dict(n_heads=nh, n_kv_heads=nkv, head_dim=hd, max_seq=max_seq, scale=0.125, theta_base=THETA)

    def call(B, kcs, vcs, positions, **kw):
        ops.attention_decode_batch(z(16 * nh * hd), z(16 * nh * hd), z(16 * nkv * hd), z(16 * nkv * hd), kcs, vcs, positions, B, **common, **kw)

    caches = mk(16)
    pos = DB.from_numpy(np.zeros(32, np.int32))
    call(1, caches[:1], caches[1:2], pos)   # (the same call, accepted)
    for B in (0, 17):
        with pytest.raises(_lib.NtkError) as e:
            call(B, caches[:8], caches[8:], pos)
        assert e.value.status == -2   # NTK_E_SHAPE
    for kw, kcs, positions in ((dict(table=False), caches[:2], pos), (dict(), [caches[0], None], pos), (dict(), caches[:2], None)):
        with pytest.raises(_lib.NtkError) as e:
            call(2, kcs, caches[2:4], positions, **kw)
        assert e.value.status == -5   # NTK_E_NULL
