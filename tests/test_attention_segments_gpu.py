"""The two kernels of the packed prompt pass through the C ABI: ntk_attention_prefill_segments against ntk_attention_prefill on every segment alone (bit
for bit) and against the oracle (the prompt-attention bar of test_hip_kernels.py::test_attention_prefill, 2e-5), ntk_rope_kv_store_segments against
ntk_rope_kv_store on every segment alone (bit for bit) and for what it must NOT write; the launchers' refusals.

Caches and Q come from one Philox key; every cache row past a segment's last key holds the half NaN 0x7E00 (rows past a prefix may hold anything:
include/ntk.h), so a finite result within the bar is also the proof that nothing past a segment's own prefix, and nothing of another segment's cache,
entered it."""
import numpy as np
import pytest

from ntransformer_amd import ops
from ntransformer_amd.ops import DeviceBuffer as DB
from test_forward_batch_cpu import segments_reference

pytestmark = pytest.mark.gpu

OK, E_SHAPE, E_NULL = 0, -2, -5
NH, NKV, MAX_SEQ = 8, 2, 256
THETA = 500000.0
NAN16 = 0x7E00
# (length, start): tile borders at 16 and 64, non-zero starts, the end of the context
SET_A = [(1, 0), (1, 37), (15, 0), (16, 64), (17, 5), (63, 1), (64, 0), (65, 127), (70, 186)]
SET_B = [(n, n - 1) for n in range(1, 17)]
SETS = {"A": SET_A, "B": SET_B}
SENTINEL = np.float32(-12345.5)

_inputs = {}


def inputs(which, hd):
    """Q [rows][NH * hd] and per segment a separately allocated (K, V) cache image: rows [0, start + n) random halves, the rest NaN.  Drawn once per
    (set, head size), shared read-only."""
    if (which, hd) not in _inputs:
        segments = SETS[which]
        r = np.random.Generator(np.random.Philox(key=[20261019, 100 * hd + len(segments)]))
        rows = sum(n for n, _ in segments)
        Q = r.standard_normal((rows, NH * hd)).astype(np.float32)
        caches = []
        for n, start in segments:
            kc, vc = (np.full(MAX_SEQ * NKV * hd, NAN16, np.uint16) for _ in range(2))
            live = (start + n) * NKV * hd
            kc[:live] = r.standard_normal(live).astype(np.float16).view(np.uint16)
            vc[:live] = r.standard_normal(live).astype(np.float16).view(np.uint16)
            caches.append((kc, vc))
        for a in [Q] + [c for pair in caches for c in pair]:
            a.setflags(write=False)
        _inputs[(which, hd)] = (Q, caches)
    return _inputs[(which, hd)]


def run_segments(Q, segments, caches, hd, order=None):
    """the segmented launch over the segments in `order` (default: as given); returns the output rows of every segment, in the GIVEN order, and the floats
    behind the output's last row"""
    order = list(range(len(segments))) if order is None else order
    row0 = np.cumsum([0] + [n for n, _ in segments])
    Qp = np.concatenate([Q[row0[s]:row0[s + 1]] for s in order])
    rows, pad = Qp.shape[0], 64
    out = np.full((rows * NH * hd + pad,), np.nan, np.float32)
    out[rows * NH * hd:] = SENTINEL
    od = DB.from_numpy(out)
    kcd = [DB.from_numpy(caches[s][0]) for s in order]
    vcd = [DB.from_numpy(caches[s][1]) for s in order]
    desc = ops.kv_segments([segments[s] for s in order], kcd, vcd)
    st = ops.attention_prefill_segments(od, DB.from_numpy(Qp), desc, NH, NKV, hd, MAX_SEQ, float(1 / np.sqrt(hd)))
    assert st == OK
    ops.synchronize()
    got = od.numpy()
    body, tail = got[: rows * NH * hd].reshape(rows, NH * hd), got[rows * NH * hd:]
    per, r = {}, 0
    for s in order:
        per[s] = body[r:r + segments[s][0]]
        r += segments[s][0]
    return [per[s] for s in range(len(segments))], tail


def single(Q, segments, caches, hd):
    """ntk_attention_prefill on every segment alone"""
    out, row = [], 0
    for (n, start), (kc, vc) in zip(segments, caches):
        od = DB.from_numpy(np.full(n * NH * hd, np.nan, np.float32))
        ops.launch_attention_prefill(od, DB.from_numpy(Q[row:row + n]), DB.from_numpy(kc), DB.from_numpy(vc), n, start, NH, NKV, hd, MAX_SEQ,
                                     float(1 / np.sqrt(hd)))
        ops.synchronize()
        out.append(od.numpy().reshape(n, NH * hd))
        row += n
    return out


@pytest.mark.parametrize("which,hd", [("A", 128), ("B", 128), ("B", 64), ("B", 256)])
def test_segments_equal_the_single_launch_bit_for_bit_and_the_oracle(which, hd):
    """head_dim 128: one launch of the matrix-core kernel's body for the segments of two rows or more + the single-query launch for single rows;
    64 / 256: ntk_attention_prefill's launch per segment.  Each segment's rows = ntk_attention_prefill on that segment alone, bit for bit; all rows
    within 2e-5 of the oracle per segment; the floats behind the last output row keep their value."""
    segments = SETS[which]
    assert which != "A" or sum(n for n, _ in segments) == 312
    Q, caches = inputs(which, hd)
    got, tail = run_segments(Q, segments, caches, hd)
    assert np.array_equal(tail, np.full(tail.shape, SENTINEL))
    want = single(Q, segments, caches, hd)
    for s, (g, w) in enumerate(zip(got, want)):
        assert np.isfinite(g).all(), (s, segments[s])
        assert np.array_equal(g.view(np.uint32), w.view(np.uint32)), (s, segments[s])
    ref = segments_reference(Q, segments, caches, NH, NKV, hd, MAX_SEQ, float(1 / np.sqrt(hd)))
    err = float(np.abs(np.concatenate(got) - ref).max())
    print(which, hd, "max |d out| against the oracle:", err)
    assert err <= 2e-5, err


@pytest.mark.parametrize("hd", [128, 64])
def test_permuting_the_segments_permutes_nothing_within_a_segment(hd):
    """Set B in another descriptor order -- other row offsets, other companions, other entries of the pointer table: the same bits per segment."""
    Q, caches = inputs("B", hd)
    order = [(5 * i + 3) % 16 for i in range(16)]
    assert sorted(order) == list(range(16))
    a, _ = run_segments(Q, SET_B, caches, hd)
    b, tail = run_segments(Q, SET_B, caches, hd, order)
    assert np.array_equal(tail, np.full(tail.shape, SENTINEL))
    for s in range(16):
        assert np.array_equal(a[s].view(np.uint32), b[s].view(np.uint32)), s


@pytest.mark.parametrize("interleaved", [0, 1])
@pytest.mark.parametrize("hd", [64, 128, 256])
@pytest.mark.parametrize("which", ["A", "B"])
def test_rope_kv_store_segments_equals_the_single_launch_and_writes_nothing_else(which, hd, interleaved):
    """q and the written cache rows = ntk_rope_kv_store on every segment alone, bit for bit; every other half of every cache keeps its sentinel."""
    segments = SETS[which]
    rows = sum(n for n, _ in segments)
    r = np.random.Generator(np.random.Philox(key=[20261019, 7 * hd + interleaved + len(segments)]))
    q = r.standard_normal((rows, NH * hd)).astype(np.float32)
    k = r.standard_normal((rows, NKV * hd)).astype(np.float32)
    v = r.standard_normal((rows, NKV * hd)).astype(np.float32)
    per = NKV * hd
    sentinel = lambda s, side: np.uint16(0x5A00 + 2 * s + side)          # a different finite half per cache
    kcd = [DB.from_numpy(np.full(MAX_SEQ * per, sentinel(s, 0), np.uint16)) for s in range(len(segments))]
    vcd = [DB.from_numpy(np.full(MAX_SEQ * per, sentinel(s, 1), np.uint16)) for s in range(len(segments))]
    qd = DB.from_numpy(q)
    st = ops.rope_kv_store_segments(qd, DB.from_numpy(k), DB.from_numpy(v), ops.kv_segments(segments, kcd, vcd), NH, NKV, hd, THETA, MAX_SEQ,
                                    interleaved=interleaved)
    assert st == OK
    ops.synchronize()
    got_q = qd.numpy().reshape(rows, NH * hd)
    row = 0
    for s, (n, start) in enumerate(segments):
        q1 = DB.from_numpy(q[row:row + n])
        k1, v1 = DB.from_numpy(np.full(MAX_SEQ * per, sentinel(s, 0), np.uint16)), DB.from_numpy(np.full(MAX_SEQ * per, sentinel(s, 1), np.uint16))
        pos = DB.from_numpy(np.arange(start, start + n, dtype=np.int32))
        ops.rope_kv_store(q1, DB.from_numpy(k[row:row + n]), DB.from_numpy(v[row:row + n]), pos, n, NH, NKV, hd, THETA, 1.0, interleaved, k1, v1, start, MAX_SEQ)
        ops.synchronize()
        assert np.array_equal(got_q[row:row + n].view(np.uint32), q1.numpy().reshape(n, NH * hd).view(np.uint32)), (s, n, start)
        for side, (mine, alone) in enumerate(((kcd[s], k1), (vcd[s], v1))):
            mine, alone = mine.numpy(np.uint16), alone.numpy(np.uint16)
            assert np.array_equal(mine, alone), (s, n, start, side)
            outside = np.concatenate([mine[: start * per], mine[(start + n) * per:]])
            assert (outside == sentinel(s, side)).all(), (s, n, start, side)
            assert (mine[start * per:(start + n) * per] != sentinel(s, side)).any()
        row += n


def test_refusals_and_a_following_valid_call():
    """Both launchers: NTK_E_SHAPE for n_seg 0 and 17 and for an overlapping row0, NTK_E_NULL for a NULL cache among the first n_seg; nothing is launched
    (q, the output and the caches keep their bytes) and the same call with a valid descriptor then works."""
    hd, per = 128, NKV * 128
    segments = [(3, 0), (2, 4)]
    r = np.random.Generator(np.random.Philox(key=[20261019, 5]))
    q = r.standard_normal((5, NH * hd)).astype(np.float32)
    kv = r.standard_normal((2, 5, per)).astype(np.float32)
    kcd = [DB.from_numpy(np.full(MAX_SEQ * per, 0x5A00, np.uint16)) for _ in range(17)]
    vcd = [DB.from_numpy(np.full(MAX_SEQ * per, 0x5A01, np.uint16)) for _ in range(17)]
    qd, kd, vd = DB.from_numpy(q), DB.from_numpy(kv[0]), DB.from_numpy(kv[1])
    od = DB.from_numpy(np.full(5 * NH * hd, SENTINEL, np.float32))
    bad = [(ops.kv_segments(segments, kcd, vcd, n_seg=0), E_SHAPE),
           (ops.kv_segments([(1, 0)] * 16, kcd, vcd, n_seg=17), E_SHAPE),
           (ops.kv_segments(segments, kcd, vcd, row0=[0, 2]), E_SHAPE),
           (ops.kv_segments(segments, [kcd[0], None], vcd), E_NULL),
           (ops.kv_segments(segments, kcd, [vcd[0], None]), E_NULL)]
    for desc, want in bad:
        assert ops.rope_kv_store_segments(qd, kd, vd, desc, NH, NKV, hd, THETA, MAX_SEQ) == want
        assert ops.attention_prefill_segments(od, qd, desc, NH, NKV, hd, MAX_SEQ, 0.1) == want
    assert ops.rope_kv_store_segments(qd, kd, vd, None, NH, NKV, hd, THETA, MAX_SEQ) == E_NULL
    assert ops.attention_prefill_segments(od, qd, None, NH, NKV, hd, MAX_SEQ, 0.1) == E_NULL
    assert ops.rope_kv_store_segments(qd, kd, vd, ops.kv_segments(segments, kcd, vcd), NH, NKV, 258, THETA, MAX_SEQ) == E_SHAPE   # head_dim > 256
    ops.synchronize()
    assert np.array_equal(qd.numpy().reshape(q.shape), q) and (od.numpy() == SENTINEL).all()
    assert (kcd[0].numpy(np.uint16) == 0x5A00).all() and (vcd[1].numpy(np.uint16) == 0x5A01).all()
    good = ops.kv_segments(segments, kcd, vcd)
    assert ops.rope_kv_store_segments(qd, kd, vd, good, NH, NKV, hd, THETA, MAX_SEQ) == OK
    assert ops.attention_prefill_segments(od, qd, good, NH, NKV, hd, MAX_SEQ, float(1 / np.sqrt(hd))) == OK
    ops.synchronize()
    out = od.numpy()
    # segment 1 starts at position 4 of a cache whose rows 0 .. 3 hold the sentinel half (finite): every output is finite and written
    assert np.isfinite(out).all() and (out != SENTINEL).all()
