"""The RoPE frequency table on the GPU, kernel by kernel: the table forms of the prompt-side rotations (ntk_rope_tab, ntk_rope_kv_store_tab,
ntk_rope_kv_store_q8_tab, ntk_rope_kv_store_segments_tab) against tests/rope_ref.py and against each other, their NULL-table case against the entry
points that have always existed, and the launches that took a table before (decode attention, context shift) given a table that carries factors.

The factor table mixes exact 1.0, ramp values and exact 8.0 over ALL pairs (rope_ref.mixed_factors), so the fast pairs are scaled too; freq_scale is 1
and 0.25.  The angle is the same F32 number on both sides -- (float)pos * tab[i] * freq_scale, left to right -- so the bar against the reference is
the one test_rope_prompt_form_is_the_per_pair_kernel_bit_for_bit has for the same sinf / cosf: 2e-5 absolute on N(0,1) data.

Run on the MI355X box:  python -m pytest tests/test_rope_table_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from ntransformer_amd import kv_ops as KO
from ntransformer_amd import kv_q8, ops
from ntransformer_amd.kv_q8 import Q8Cache
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O
from rope_ref import mixed_factors, rope_ref, scaled_table

pytestmark = pytest.mark.gpu
THETA = 500000.0
SHAPES = [(8, 2, 64), (32, 8, 128), (4, 4, 256)]
PAIR_SHAPES = SHAPES + [(2, 1, 80)]
EDGE = [0, 1, 4095, 131071]


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261020, seed]))


def table(hd):
    return scaled_table(hd, THETA, mixed_factors(hd, hd))


def positions_for(T, r):
    if T == 1:
        return [131071]
    if T == 3:
        return [0, 1, 131071]
    return EDGE + [int(p) for p in r.integers(0, 131072, T - 4)]


def qkv(r, T, nh, nkv, hd):
    return (r.standard_normal(T * nh * hd).astype(np.float32), r.standard_normal(T * nkv * hd).astype(np.float32),
            r.standard_normal(T * nkv * hd).astype(np.float32))


def rope_tab(q, k, positions, nh, nkv, hd, fscale, interleaved, tab):
    qd, kd = DB.from_numpy(q), DB.from_numpy(k)
    ops.rope_tab(qd, kd, DB.from_numpy(np.asarray(positions, np.int32)), len(positions), nh, nkv, hd, THETA, fscale, interleaved,
                 None if tab is None else DB.from_numpy(tab))
    ops.synchronize()
    return qd.numpy().copy(), kd.numpy().copy()


# ------------------------------------------------------------------------------------------------ 1, 2: ntk_rope_tab
@pytest.mark.parametrize("fscale", [1.0, 0.25])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("nh,nkv,hd", PAIR_SHAPES)
def test_rope_tab_both_forms_against_the_reference(nh, nkv, hd, interleaved, fscale):
    """per-pair form (T = 1, 3; every edge position alone as well) and rows form (T = 4, 37)"""
    tab = table(hd)
    r = rng(hd + nh + interleaved)
    cases = [(1, [p]) for p in EDGE] + [(T, positions_for(T, r)) for T in (3, 4, 37)]
    for T, positions in cases:
        q, k, _ = qkv(r, T, nh, nkv, hd)
        got_q, got_k = rope_tab(q, k, positions, nh, nkv, hd, fscale, interleaved, tab)
        want_q, want_k = rope_ref(q, k, positions, nh, nkv, hd, tab, fscale, interleaved)
        eq, ek = float(np.abs(got_q - want_q).max()), float(np.abs(got_k - want_k).max())
        print("rope_tab %d/%d/%d T %d interleaved %d fscale %g: |dq| %.3g |dk| %.3g" % (nh, nkv, hd, T, interleaved, fscale, eq, ek))
        assert eq <= 2e-5 and ek <= 2e-5, (T, positions[:4], eq, ek)
        if max(positions) >= 4095:   # the table is not ignored: the unscaled rotation is somewhere else
            plain_q, _ = rope_tab(q, k, positions, nh, nkv, hd, 1.0, interleaved, None)
            assert np.abs(plain_q - got_q).max() > 1e-2


@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("nh,nkv,hd", PAIR_SHAPES)
def test_rope_tab_rows_form_is_the_per_pair_form_bit_for_bit(nh, nkv, hd, interleaved):
    tab, T, fscale = table(hd), 37, 0.25
    r = rng(100 + hd + interleaved)
    positions = positions_for(T, r)
    q, k, _ = qkv(r, T, nh, nkv, hd)
    got_q, got_k = rope_tab(q, k, positions, nh, nkv, hd, fscale, interleaved, tab)
    for t in range(T):
        one_q, one_k = rope_tab(q[t * nh * hd:(t + 1) * nh * hd], k[t * nkv * hd:(t + 1) * nkv * hd], [positions[t]], nh, nkv, hd, fscale, interleaved, tab)
        assert np.array_equal(got_q[t * nh * hd:(t + 1) * nh * hd].view(np.uint32), one_q.view(np.uint32)), t
        assert np.array_equal(got_k[t * nkv * hd:(t + 1) * nkv * hd].view(np.uint32), one_k.view(np.uint32)), t


# ------------------------------------------------------------------------------------------------ 3: NULL table = the existing entry points
@pytest.mark.parametrize("nh,nkv,hd", PAIR_SHAPES)
def test_null_table_gives_the_existing_entry_points_bits(nh, nkv, hd):
    r = rng(200 + hd)
    max_seq, start = 64, 9
    for T, interleaved, fscale in [(1, False, 1.0), (3, True, 0.25), (4, False, 0.25), (37, True, 1.0)]:
        positions = positions_for(T, r)
        q, k, v = qkv(r, T, nh, nkv, hd)
        pd = DB.from_numpy(np.asarray(positions, np.int32))
        a_q, a_k = DB.from_numpy(q), DB.from_numpy(k)
        ops.launch_rope(a_q, a_k, pd, 1, T, nh, nkv, hd, THETA, fscale, interleaved)
        b_q, b_k = rope_tab(q, k, positions, nh, nkv, hd, fscale, interleaved, None)
        assert np.array_equal(a_q.numpy().view(np.uint32), b_q.view(np.uint32)) and np.array_equal(a_k.numpy().view(np.uint32), b_k.view(np.uint32))
        junk = r.integers(0, 65536, max_seq * nkv * hd).astype(np.uint16)
        out = []
        for tabbed in (False, True):
            qd, kc, vc = DB.from_numpy(q), DB.from_numpy(junk), DB.from_numpy(junk[::-1].copy())
            if tabbed:
                ops.rope_kv_store_tab(qd, DB.from_numpy(k), DB.from_numpy(v), pd, T, nh, nkv, hd, THETA, fscale, interleaved, kc, vc, start, max_seq, None)
            else:
                ops.rope_kv_store(qd, DB.from_numpy(k), DB.from_numpy(v), pd, T, nh, nkv, hd, THETA, fscale, interleaved, kc, vc, start, max_seq)
            ops.synchronize()
            out.append((qd.numpy().view(np.uint32).copy(), kc.numpy(np.uint16).copy(), vc.numpy(np.uint16).copy()))
        assert all(np.array_equal(x, y) for x, y in zip(*out))
        # ... the segmented launch
        segs = [(T, start)]
        out = []
        for tabbed in (False, True):
            qd, kc, vc = DB.from_numpy(q), DB.from_numpy(junk), DB.from_numpy(junk[::-1].copy())
            fn = ops.rope_kv_store_segments_tab if tabbed else ops.rope_kv_store_segments
            assert fn(qd, DB.from_numpy(k), DB.from_numpy(v), ops.kv_segments(segs, [kc], [vc]), nh, nkv, hd, THETA, max_seq, freq_scale=fscale,
                      interleaved=interleaved) == 0
            ops.synchronize()
            out.append((qd.numpy().view(np.uint32).copy(), kc.numpy(np.uint16).copy(), vc.numpy(np.uint16).copy()))
        assert all(np.array_equal(x, y) for x, y in zip(*out))
        if hd % 32 == 0:   # ... the 8-bit store
            out = []
            for tabbed in (False, True):
                qd, kc, vc = DB.from_numpy(q), Q8Cache(max_seq, nkv, hd, fill=0x11), Q8Cache(max_seq, nkv, hd, fill=0x22)
                fn = kv_q8.rope_kv_store_q8_tab if tabbed else kv_q8.rope_kv_store_q8
                fn(qd, DB.from_numpy(k), DB.from_numpy(v), pd, T, nh, nkv, hd, THETA, kc, vc, start, freq_scale=fscale, interleaved=int(interleaved))
                ops.synchronize()
                out.append((qd.numpy().view(np.uint32).copy(), kc.raw().copy(), vc.raw().copy()))
            assert all(np.array_equal(x, y) for x, y in zip(*out))


# ------------------------------------------------------------------------------------------------ 4, 5: the fused stores = rope_tab + store
@pytest.mark.parametrize("fscale", [1.0, 0.25])
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_rope_kv_store_tab_equals_rope_tab_then_copy_to_kv_cache(nh, nkv, hd, interleaved, fscale):
    """q and both caches bit for bit; every byte outside the written rows keeps what it held"""
    tab, max_seq = table(hd), 64
    r = rng(300 + hd + interleaved)
    for T, start in [(4, 0), (37, 21)]:
        positions = positions_for(T, r)
        q, k, v = qkv(r, T, nh, nkv, hd)
        pd, td = DB.from_numpy(np.asarray(positions, np.int32)), DB.from_numpy(tab)
        junk = r.integers(0, 65536, max_seq * nkv * hd).astype(np.uint16)
        q1, k1 = DB.from_numpy(q), DB.from_numpy(k)
        kc1, vc1 = DB.from_numpy(junk), DB.from_numpy(junk[::-1].copy())
        ops.rope_tab(q1, k1, pd, T, nh, nkv, hd, THETA, fscale, interleaved, td)
        ops.launch_copy_to_kv_cache(kc1, vc1, k1, DB.from_numpy(v), T, nkv, hd, start, max_seq)
        q2, k2, v2 = DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v)
        kc2, vc2 = DB.from_numpy(junk), DB.from_numpy(junk[::-1].copy())
        ops.rope_kv_store_tab(q2, k2, v2, pd, T, nh, nkv, hd, THETA, fscale, interleaved, kc2, vc2, start, max_seq, td)
        ops.synchronize()
        assert np.array_equal(q1.numpy().view(np.uint32), q2.numpy().view(np.uint32))
        assert np.array_equal(k2.numpy(), k) and np.array_equal(v2.numpy(), v)                     # k, v only read
        got_k, got_v = kc2.numpy(np.uint16), vc2.numpy(np.uint16)
        assert np.array_equal(kc1.numpy(np.uint16), got_k) and np.array_equal(vc1.numpy(np.uint16), got_v)
        per = nkv * hd
        outside = np.ones(max_seq * per, bool)
        outside[start * per:(start + T) * per] = False
        assert np.array_equal(got_k[outside], junk[outside]) and np.array_equal(got_v[outside], junk[::-1][outside])
        want_q, want_k = rope_ref(q, k, positions, nh, nkv, hd, tab, fscale, interleaved)          # ... and they are the scaled rotation
        assert np.abs(q2.numpy() - want_q).max() <= 2e-5
        stored = got_k[start * per:(start + T) * per].view(np.float16).astype(np.float32)
        assert np.abs(stored - want_k).max() <= 2e-3 * max(1.0, float(np.abs(want_k).max()))


@pytest.mark.parametrize("fscale", [1.0, 0.25])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_rope_kv_store_q8_tab_equals_rope_tab_then_kv_store_q8(nh, nkv, hd, fscale):
    tab, max_seq = table(hd), 64
    r = rng(400 + hd)
    for T, start, interleaved in [(4, 0, True), (37, 21, False)]:
        positions = positions_for(T, r)
        q, k, v = qkv(r, T, nh, nkv, hd)
        pd, td = DB.from_numpy(np.asarray(positions, np.int32)), DB.from_numpy(tab)
        qa, ka, va = DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v)
        kca, vca = Q8Cache(max_seq, nkv, hd, fill=0x11), Q8Cache(max_seq, nkv, hd, fill=0x22)
        ops.rope_tab(qa, ka, pd, T, nh, nkv, hd, THETA, fscale, interleaved, td)
        kv_q8.kv_store_q8(kca, vca, ka, va, T, nkv, hd, start)
        qb, kb = DB.from_numpy(q), DB.from_numpy(k)
        kcb, vcb = Q8Cache(max_seq, nkv, hd, fill=0x11), Q8Cache(max_seq, nkv, hd, fill=0x22)
        kv_q8.rope_kv_store_q8_tab(qb, kb, va, pd, T, nh, nkv, hd, THETA, kcb, vcb, start, freq_scale=fscale, interleaved=int(interleaved), inv_freq=td)
        ops.synchronize()
        assert np.array_equal(qa.numpy().view(np.uint32), qb.numpy().view(np.uint32))
        assert np.array_equal(kb.numpy(), k)
        assert np.array_equal(kca.raw(), kcb.raw()) and np.array_equal(vca.raw(), vcb.raw())
        assert kcb.read_blocks(start, T).any()


# ------------------------------------------------------------------------------------------------ 6: segments
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("nh,nkv,hd", SHAPES)
def test_rope_kv_store_segments_tab_equals_the_single_sequence_launch_per_segment(nh, nkv, hd, interleaved):
    tab, max_seq, fscale = table(hd), 4200, 0.25
    segments = [(5, 0), (1, 4095), (9, 130)]          # different start positions and caches; a one-row segment
    rows, per = sum(n for n, _ in segments), nkv * hd
    r = rng(500 + hd + interleaved)
    q, k, v = (x.reshape(rows, -1) for x in qkv(r, rows, nh, nkv, hd))
    td = DB.from_numpy(tab)
    sentinel = lambda s, side: np.uint16(0x5A00 + 2 * s + side)
    kcd = [DB.from_numpy(np.full(max_seq * per, sentinel(s, 0), np.uint16)) for s in range(len(segments))]
    vcd = [DB.from_numpy(np.full(max_seq * per, sentinel(s, 1), np.uint16)) for s in range(len(segments))]
    qd = DB.from_numpy(q)
    assert ops.rope_kv_store_segments_tab(qd, DB.from_numpy(k), DB.from_numpy(v), ops.kv_segments(segments, kcd, vcd), nh, nkv, hd, THETA, max_seq,
                                          freq_scale=fscale, interleaved=interleaved, inv_freq=td) == 0
    ops.synchronize()
    got_q = qd.numpy().reshape(rows, nh * hd)
    row = 0
    for s, (n, start) in enumerate(segments):
        q1 = DB.from_numpy(q[row:row + n])
        k1, v1 = DB.from_numpy(np.full(max_seq * per, sentinel(s, 0), np.uint16)), DB.from_numpy(np.full(max_seq * per, sentinel(s, 1), np.uint16))
        pos = DB.from_numpy(np.arange(start, start + n, dtype=np.int32))
        ops.rope_kv_store_tab(q1, DB.from_numpy(k[row:row + n]), DB.from_numpy(v[row:row + n]), pos, n, nh, nkv, hd, THETA, fscale, interleaved, k1, v1, start,
                              max_seq, td)
        ops.synchronize()
        assert np.array_equal(got_q[row:row + n].view(np.uint32), q1.numpy().reshape(n, nh * hd).view(np.uint32)), s
        assert np.array_equal(kcd[s].numpy(np.uint16), k1.numpy(np.uint16)) and np.array_equal(vcd[s].numpy(np.uint16), v1.numpy(np.uint16)), s
        want_q, _ = rope_ref(q[row:row + n].reshape(-1), k[row:row + n].reshape(-1), list(range(start, start + n)), nh, nkv, hd, tab, fscale, interleaved)
        assert np.abs(got_q[row:row + n].reshape(-1) - want_q).max() <= 2e-5
        row += n


# ------------------------------------------------------------------------------------------------ 7: the decode launches
@pytest.mark.parametrize("fscale", [1.0, 0.25])
@pytest.mark.parametrize("pos,nh,nkv,hd,nsplit", [(300, 32, 8, 128, 0), (2047, 32, 8, 128, 32), (700, 8, 2, 64, 8), (63, 4, 4, 256, 0), (1100, 32, 8, 128, 8)])
def test_decode_attention_with_a_factor_table(pos, nh, nkv, hd, nsplit, fscale):
    """ntk_attention_decode_fused (nsplit 0) / ntk_attention_decode_split given a table with factors: rope_ref + the oracle's store + the oracle's
    attention; the bars of test_attention_decode_fused_equals_rope_store_attend"""
    tab = table(hd)
    r = rng(600 + pos + hd)
    max_seq = 2048
    kc = np.zeros(max_seq * nkv * hd, np.uint16)
    vc = np.zeros(max_seq * nkv * hd, np.uint16)
    kc[: pos * nkv * hd] = r.standard_normal(pos * nkv * hd).astype(np.float16).view(np.uint16)
    vc[: pos * nkv * hd] = r.standard_normal(pos * nkv * hd).astype(np.float16).view(np.uint16)
    q, k, v = qkv(r, 1, nh, nkv, hd)
    scale = float(1 / np.sqrt(hd))
    rq, rk = rope_ref(q, k, [pos], nh, nkv, hd, tab, fscale)
    kc_ref, vc_ref = kc.copy(), vc.copy()
    O.copy_to_kv_cache(kc_ref, vc_ref, rk, v, 1, nkv, hd, pos, max_seq)
    ref = O.attention_decode(rq, kc_ref, vc_ref, pos + 1, nh, nkv, hd, max_seq, scale)
    kcd, vcd = DB.from_numpy(kc), DB.from_numpy(vc)
    od = DB.from_numpy(np.full(nh * hd, np.nan, np.float32))
    args = (od, DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v), kcd, vcd, DB.from_numpy(np.array([pos], np.int32)), nh, nkv, hd, max_seq, scale, THETA)
    if nsplit:
        ops.attention_decode_split(*args, nsplit, freq_scale=fscale, inv_freq=DB.from_numpy(tab))
    else:
        ops.attention_decode_fused(*args, freq_scale=fscale, inv_freq=DB.from_numpy(tab))
    ops.synchronize()
    assert np.abs(od.numpy() - ref).max() <= 3e-5
    assert np.array_equal(vcd.numpy(np.uint16), vc_ref)
    got_k = kcd.numpy(np.uint16).view(np.float16).astype(np.float32)
    want_k = kc_ref.view(np.float16).astype(np.float32)
    assert np.abs(got_k - want_k).max() <= 2e-3 * max(1.0, np.abs(want_k).max())
    uq, uk = O.rope(q, k, [pos], nh, nkv, hd, THETA)          # the unscaled rotation is somewhere else
    assert np.abs(uk - rk).max() > 1e-2


# ------------------------------------------------------------------------------------------------ 8: the context shift
@pytest.mark.parametrize("fscale", [1.0, 0.25])
@pytest.mark.parametrize("interleaved", [False, True])
def test_kv_shift_with_a_factor_table(interleaved, fscale):
    """ntk_kv_shift given a table with factors against kv_ops.shift_f16_ref given the same table, at test_kv_shift_f16_against_the_checker's bar"""
    L, S, nkv, hd = 2, 96, 2, 128
    src0, dst0, n = 8, 4, 40
    r = rng(700 + interleaved)
    k0 = r.standard_normal((L, S, nkv * hd)).astype(np.float16).view(np.uint16)
    v0 = r.standard_normal((L, S, nkv * hd)).astype(np.float16).view(np.uint16)
    tab = table(hd)
    kd, vd = DB.from_numpy(k0), DB.from_numpy(v0)
    KO.kv_shift(kd, vd, L, S, nkv, hd, src0, dst0, n, inv_freq=DB.from_numpy(tab), theta_base=THETA, freq_scale=fscale, interleaved=interleaved)
    ops.synchronize()
    k1, v1 = kd.numpy(np.uint16).reshape(k0.shape), vd.numpy(np.uint16).reshape(v0.shape)
    want_k, want_v = KO.shift_f16_ref(k0, v0, src0, dst0, n, hd, inv_freq=tab, freq_scale=fscale, interleaved=interleaved)
    assert np.array_equal(v1, want_v)
    outside = np.ones(S, bool)
    outside[dst0:dst0 + n] = False
    assert np.array_equal(k1[:, outside], k0[:, outside])
    got = k1[:, dst0:dst0 + n].view(np.float16).astype(np.float64)
    want = want_k[:, dst0:dst0 + n].view(np.float16).astype(np.float64)
    bar = 2.0 ** -10 * KO.pair_max(k0[:, src0:src0 + n].view(np.float16), hd, interleaved) + 2.0 ** -24
    assert (np.abs(got - want) <= bar).all()
    plain_k, _ = KO.shift_f16_ref(k0, v0, src0, dst0, n, hd, theta=THETA, interleaved=interleaved)
    assert np.abs(plain_k[:, dst0:dst0 + n].view(np.float16).astype(np.float64) - want).max() > 1e-2
