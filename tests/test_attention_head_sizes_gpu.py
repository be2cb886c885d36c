"""The attention family at the head sizes other than the everyday 128, every form through the C ABI against the oracle.

The kernels are written for four head-size classes -- 128, 64 (LPR 8), 256 (LPR 32) and "any even size" (LPR 0, the three-pass `attend`) -- and the
sizes other than 128 contain code only they execute: at 256 the second rotation pair and the second V element per thread of attention_decode_walk,
its in-kernel frequency for that pair, groups of 2 positions per wave instruction, the second trip of the combine loop, waves 2 and 3 of the merging
workgroup, the 96 KiB tiled prompt kernel; on the generic path the causal prompt kernel with several queries and the score row beyond 64 KiB of LDS.

  class     (heads, KV heads, head size)
  256       (8, 2, 256) (4, 4, 256) (16, 1, 256)            GQA 4 / 1 / 16
  64        (8, 2, 64) (5, 1, 64) (8, 8, 64)
  generic   (6, 3, 80) (4, 2, 96)
  generic   (8, 2, 128), the cache pointers 8 bytes off 16-byte alignment: the `aligned` = false route to LPR 0

Inputs: N(0, 1) halves in the cache rows below the position; EVERY row from the position on holds NaN / inf / junk halves (test_attention_batch_gpu.py's
JUNK), and max_seq carries a slack of a few dozen rows, so a result inside the bar is also the proof that clamped and prefetched rows took no part.
After each launch the whole cache apart from the written row is compared bit for bit with what was uploaded.

Positions come from the walk's own geometry: LPR = hd / 8, G = 4 (64 / LPR) position groups, a whole batch = 4 G nsplit positions (positions()),
and at (4, 4, 256) and (8, 2, 64) every position 0 .. 2 G nsplit + 1, which walks the new token's turn through every group and split.

The reference of a decode step is the oracle's rope + copy_to_kv_cache + attention_decode.  Bars (test_hip_kernels.py's, named at each assertion):
2e-5 for the 1:1 and prompt kernels (x max(1, |ref|max) where Q is scaled, as in test_attention_prefill_mfma_random_sweep), 3e-5 for fused / split
against the oracle, 2e-6 for split against the single pass, the stored V bit for bit, the stored K within 2e-3 max(1, |K|max), bits equal for merged
against two-launch and for segments against single launches.

With NTK_HEAD_SIZE_PARITY_OUT=<file> in the environment the largest deviation per form and head size is written there when the module finishes
(profiles/head_size_parity.txt is such a run)."""
import functools
import os

import numpy as np
import pytest

from ntransformer_amd import _lib, ops
from ntransformer_amd import engine as E
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O
from rope_ref import rope_ref, scaled_table
from test_attention_batch_gpu import THETA, _halves, _inv_freq, _junk
import test_attention_segments_gpu as SEG

pytestmark = pytest.mark.gpu

E_SHAPE, E_ALIGN = -2, -4
HD256 = [(8, 2, 256), (4, 4, 256), (16, 1, 256)]
HD64 = [(8, 2, 64), (5, 1, 64), (8, 8, 64)]
GENERIC = [(6, 3, 80), (4, 2, 96)]
# (heads, KV heads, head size, bytes the cache pointers are moved off their 16-byte alignment)
WALK = [g + (0,) for g in HD256 + HD64]
ANY = [g + (0,) for g in GENERIC] + [(8, 2, 128, 8)]
ALL = WALK + ANY
gid = lambda g: "%d-%d-%d%s" % (g[0], g[1], g[2], "-unaligned" if g[3] else "")

_worst = {}


def note(form, hd, err, bar):
    """the largest deviation seen per (form, head size), with its bar"""
    key = (form, hd)
    _worst[key] = (max(err, _worst.get(key, (0.0, bar))[0]), bar)


@pytest.fixture(scope="module", autouse=True)
def _parity_file():
    yield
    path = os.environ.get("NTK_HEAD_SIZE_PARITY_OUT")
    if path and _worst:
        with open(path, "w") as f:
            for (form, hd), (err, bar) in sorted(_worst.items()):
                f.write("%-52s head_dim %3d   max deviation %.3e   bar %.1e\n" % (form, hd, err, bar))


def walk_geometry(hd, nsplit):
    """(G, positions of a whole batch) of attention_decode_walk<LPR, 4>; the generic sizes get the same formula (any position serves there)"""
    G = 4 * (64 // (hd // 8))
    return G, 4 * G * nsplit


def positions(hd, nsplit):
    G, batch = walk_geometry(hd, nsplit)
    return sorted({0, 1, G - 1, G, G + 1, batch - 1, batch, batch + 1, 3 * batch + G + 1, 543, 544, 2047})


class Cache:
    """a cache image on the device, optionally `shift` bytes off the allocation's alignment"""

    def __init__(self, image, shift=0):
        self.n, self.shift = image.size, shift
        self.buf = DB(image.nbytes + 16)
        self.buf.upload(image, shift)
        self.ptr = self.buf.at(shift)

    def read(self):
        return self.buf.numpy(np.uint16, self.n, self.shift)


@functools.lru_cache(maxsize=24)
def step_case(nh, nkv, hd, pos):
    """One decode step's inputs and the oracle's answer, shared by the forms (read only): q, k, v, the cache images (rows [0, pos) N(0, 1), the
    rest junk), max_seq, and the oracle's output and caches after rope + copy_to_kv_cache + attention_decode."""
    max_seq = pos + 1 + (7 * nh + hd + 13 * pos) % 47 + 3
    row = nkv * hd
    seed = 100000 * nh + 1000 * (hd % 97) + pos
    r = np.random.default_rng(seed)
    q = r.standard_normal(nh * hd).astype(np.float32)
    k = r.standard_normal(row).astype(np.float32)
    v = r.standard_normal(row).astype(np.float32)
    kc, vc = _junk(max_seq * row, seed).copy(), _junk(max_seq * row, seed + 1).copy()
    kc[: pos * row] = _halves(pos * row, seed)
    vc[: pos * row] = _halves(pos * row, seed + 1)
    ref, kc_ref, vc_ref = oracle_step(q, k, v, kc, vc, pos, nh, nkv, hd, max_seq)
    for a in (q, k, v, kc, vc, ref, kc_ref, vc_ref):
        a.setflags(write=False)
    return q, k, v, kc, vc, max_seq, ref, kc_ref, vc_ref


def oracle_step(q, k, v, kc, vc, pos, nh, nkv, hd, max_seq, tab=None):
    rq, rk = O.rope(q, k, [pos], nh, nkv, hd, THETA) if tab is None else rope_ref(q, k, [pos], nh, nkv, hd, tab)
    kc_ref, vc_ref = kc.copy(), vc.copy()
    O.copy_to_kv_cache(kc_ref, vc_ref, rk, v, 1, nkv, hd, pos, max_seq)
    ref = O.attention_decode(rq, kc_ref, vc_ref, pos + 1, nh, nkv, hd, max_seq, float(1 / np.sqrt(hd)))
    return ref, kc_ref, vc_ref


def launch_step(form, q, k, v, kc, vc, pos, nh, nkv, hd, max_seq, shift=0, nsplit=1, inv=None):
    """one launch of `form` ("fused", "split", "merged": three launches on one scratch) on fresh device copies; (out, K cache, V cache) read back"""
    kcd, vcd = Cache(kc, shift), Cache(vc, shift)
    od = DB.from_numpy(np.full(nh * hd, np.nan, np.float32))
    args = (od, DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v), kcd.ptr, vcd.ptr, DB.from_numpy(np.array([pos], np.int32)),
            nh, nkv, hd, max_seq, float(1 / np.sqrt(hd)), THETA)
    if form == "fused": ops.attention_decode_fused(*args, inv_freq=inv)
    elif form == "split": ops.attention_decode_split(*args, nsplit, inv_freq=inv)
    else: ops.attention_decode_split_merged(*args, nsplit, inv_freq=inv, launches=3)
    return od.numpy(), kcd.read(), vcd.read()


def check_step(form, got, ref, kc_ref, vc_ref, kc, vc, pos, nkv, hd, what):
    """the bars of test_attention_decode_fused_equals_rope_store_attend, and: nothing but the position's row changed"""
    out, got_k, got_v = got
    assert np.isfinite(out).all(), what
    err = float(np.abs(out - ref).max())
    note(form + " against the oracle", hd, err, 3e-5)
    assert err <= 3e-5, (what, err)
    row = nkv * hd
    new = slice(pos * row, (pos + 1) * row)
    assert np.array_equal(got_v[new], vc_ref[new]), what                                      # V: bit for bit
    gk, wk = got_k[new].view(np.float16).astype(np.float32), kc_ref[new].view(np.float16).astype(np.float32)
    assert np.abs(gk - wk).max() <= 2e-3 * max(1.0, float(np.abs(wk).max())), what            # K: device against glibc sin / cos
    for g, was in ((got_k, kc), (got_v, vc)):
        assert np.array_equal(g[: pos * row], was[: pos * row]) and np.array_equal(g[(pos + 1) * row:], was[(pos + 1) * row:]), what


# ------------------------------------------------------------------------------------------------ the 1:1 kernel
@pytest.mark.parametrize("seq", [1, 17, 140, 1025])
@pytest.mark.parametrize("geom", ALL, ids=gid)
def test_attention_decode_1to1(geom, seq):
    """ntk_attention_decode (attention_kernel<8 | 32 | 0>, one query) against oracle.attention_decode, 2e-5 (test_attention_decode); it writes nothing"""
    nh, nkv, hd, shift = geom
    q, _, _, kc, vc, max_seq, _, _, _ = step_case(nh, nkv, hd, seq)          # rows [0, seq) live, junk behind them
    scale = float(1 / np.sqrt(hd))
    ref = O.attention_decode(q, kc, vc, seq, nh, nkv, hd, max_seq, scale)
    kcd, vcd = Cache(kc, shift), Cache(vc, shift)
    od = DB.from_numpy(np.full(nh * hd, np.nan, np.float32))
    ops.launch_attention_decode(od, DB.from_numpy(q), kcd.ptr, vcd.ptr, seq, nh, nkv, hd, max_seq, scale)
    out = od.numpy()
    assert np.isfinite(out).all()
    err = float(np.abs(out - ref).max())
    note("ntk_attention_decode against the oracle", hd, err, 2e-5)
    assert err <= 2e-5, err
    assert np.array_equal(kcd.read(), kc) and np.array_equal(vcd.read(), vc)


# ------------------------------------------------------------------------------------------------ the fused step
@pytest.mark.parametrize("table", [False, True], ids=["in-kernel-frequency", "table"])
@pytest.mark.parametrize("geom", ALL, ids=gid)
def test_attention_decode_fused(geom, table):
    """ntk_attention_decode_fused at the positions of the walk's geometry, with the in-kernel frequency (at 256: the `pow` of the second pair too) and
    with the host's F32 table (the generic kernel computes its own frequency either way)"""
    nh, nkv, hd, shift = geom
    inv = DB.from_numpy(_inv_freq(hd)) if table else None
    for pos in positions(hd, 1):
        q, k, v, kc, vc, max_seq, ref, kc_ref, vc_ref = step_case(nh, nkv, hd, pos)
        got = launch_step("fused", q, k, v, kc, vc, pos, nh, nkv, hd, max_seq, shift, inv=inv)
        check_step("fused", got, ref, kc_ref, vc_ref, kc, vc, pos, nkv, hd, (geom, table, pos))


@pytest.mark.parametrize("nsplit", [0, 8])
@pytest.mark.parametrize("geom", [WALK[0], WALK[3]], ids=gid)
def test_attention_decode_with_llama3_factors(geom, nsplit):
    """A Llama-3 factor table (the engine's own: rope_llama3_factors over the correctly rounded frequencies) in the fused (nsplit 0) and the split
    launch: rope_ref + the oracle's store and attention.  At 256 the second pair reads inv_freq[ri + 64]: pairs 64 .. 127 are the slow ones the
    factors divide by 8."""
    nh, nkv, hd, _ = geom
    factors = E.rope_llama3_factors(hd, THETA)
    assert factors.min() == 1.0 and factors.max() == 8.0
    tab = scaled_table(hd, THETA, factors)
    for pos in (1, 63, 544, 2047):
        q, k, v, kc, vc, max_seq, _, _, _ = step_case(nh, nkv, hd, pos)
        ref, kc_ref, vc_ref = oracle_step(q, k, v, kc, vc, pos, nh, nkv, hd, max_seq, tab)
        got = launch_step("split" if nsplit else "fused", q, k, v, kc, vc, pos, nh, nkv, hd, max_seq, nsplit=nsplit, inv=DB.from_numpy(tab))
        check_step("factor table, fused / split", got, ref, kc_ref, vc_ref, kc, vc, pos, nkv, hd, (geom, nsplit, pos))
        if pos == 2047:   # (the unscaled rotation is somewhere else)
            new = slice(pos * nkv * hd, (pos + 1) * nkv * hd)
            plain = step_case(nh, nkv, hd, pos)[7][new].view(np.float16).astype(np.float32)
            assert np.abs(kc_ref[new].view(np.float16).astype(np.float32) - plain).max() > 1e-2


# ------------------------------------------------------------------------------------------------ the split forms
def split_against_oracle_and_single_pass(nh, nkv, hd, nsplit, pos, merged=False):
    q, k, v, kc, vc, max_seq, ref, kc_ref, vc_ref = step_case(nh, nkv, hd, pos)
    what = (nh, nkv, hd, nsplit, pos)
    got = launch_step("split", q, k, v, kc, vc, pos, nh, nkv, hd, max_seq, nsplit=nsplit)
    check_step("split", got, ref, kc_ref, vc_ref, kc, vc, pos, nkv, hd, what)
    one = launch_step("fused", q, k, v, kc, vc, pos, nh, nkv, hd, max_seq)
    d = float(np.abs(got[0] - one[0]).max())
    note("split against the single pass", hd, d, 2e-6)
    assert d <= 2e-6, (what, d)                                                # test_attention_decode_split_equals_oracle_and_single_pass
    assert np.array_equal(got[1], one[1]) and np.array_equal(got[2], one[2]), what
    if merged:   # three launches on one scratch: the bits of the two-launch form, hence inside the oracle bar as well
        m = launch_step("merged", q, k, v, kc, vc, pos, nh, nkv, hd, max_seq, nsplit=nsplit)
        assert np.array_equal(m[0].view(np.uint32), got[0].view(np.uint32)), what
        assert np.array_equal(m[1], got[1]) and np.array_equal(m[2], got[2]), what
        check_step("merged split", m, ref, kc_ref, vc_ref, kc, vc, pos, nkv, hd, what)


@pytest.mark.parametrize("nsplit", [1, 3, 8, 16, 17])
@pytest.mark.parametrize("geom", WALK, ids=gid)
def test_attention_decode_split(geom, nsplit):
    """ntk_attention_decode_split (the walk with SPLIT, then attention_split_combine_head: at 256 its 128 threads make a second trip) at the positions
    of the walk's geometry for this split count; 3 and 17 splits exceed the position count of the small cases"""
    nh, nkv, hd, _ = geom
    for pos in positions(hd, nsplit):
        split_against_oracle_and_single_pass(nh, nkv, hd, nsplit, pos)


@pytest.mark.parametrize("nsplit", [8, 16])
@pytest.mark.parametrize("geom", WALK, ids=gid)
def test_attention_decode_split_merged(geom, nsplit):
    """ntk_attention_decode_split_merged (at 256, waves 2 and 3 of the last workgroup merge as well): bit for bit the two-launch form, which the same
    call pins to the oracle"""
    nh, nkv, hd, _ = geom
    for pos in positions(hd, nsplit):
        split_against_oracle_and_single_pass(nh, nkv, hd, nsplit, pos, merged=True)


@pytest.mark.parametrize("pos,nh,nkv,hd,nsplit", [(900, 8, 8, 256, 8), (700, 12, 4, 64, 5), (1023, 16, 16, 128, 33), (2500, 40, 8, 128, 64)])
def test_attention_decode_split_at_the_merged_tests_shapes(pos, nh, nkv, hd, nsplit):
    """The shapes test_attention_decode_split_merged_equals_the_two_launch_form (test_hip_kernels.py) compares with the two-launch form only: that form
    against the oracle and the single pass here, and the merged one with it."""
    split_against_oracle_and_single_pass(nh, nkv, hd, nsplit, pos, merged=True)


@pytest.mark.parametrize("nsplit", [1, 3])
@pytest.mark.parametrize("geom", [WALK[1], WALK[3]], ids=gid)
def test_attention_decode_every_residue_of_the_position(geom, nsplit):
    """Every position 0 .. 2 G nsplit + 1: the new token is taken "by the group whose turn it is" (first + g == pos % stepG), and this walks that turn
    through every group of every split, twice; one split: the fused launch as well"""
    nh, nkv, hd, _ = geom
    G, _ = walk_geometry(hd, nsplit)
    for pos in range(2 * G * nsplit + 2):
        split_against_oracle_and_single_pass(nh, nkv, hd, nsplit, pos)


@pytest.mark.parametrize("geom", ANY, ids=gid)
def test_attention_decode_split_refuses_the_generic_sizes(geom):
    """head sizes 80 / 96: NTK_E_SHAPE; head size 128 on caches off 16-byte alignment: NTK_E_ALIGN; both forms, output and caches untouched"""
    nh, nkv, hd, shift = geom
    q, k, v, kc, vc, max_seq, _, _, _ = step_case(nh, nkv, hd, 140)
    kcd, vcd = Cache(kc, shift), Cache(vc, shift)
    od = DB.from_numpy(np.full(nh * hd, -7.5, np.float32))
    args = (od, DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v), kcd.ptr, vcd.ptr, DB.from_numpy(np.array([140], np.int32)),
            nh, nkv, hd, max_seq, float(1 / np.sqrt(hd)), THETA, 8)
    for launch in (ops.attention_decode_split, ops.attention_decode_split_merged):
        with pytest.raises(_lib.NtkError) as e:
            launch(*args)
        assert e.value.status == (E_ALIGN if shift else E_SHAPE)
    ops.synchronize()
    assert (od.numpy() == -7.5).all() and np.array_equal(kcd.read(), kc) and np.array_equal(vcd.read(), vc)


# ------------------------------------------------------------------------------------------------ the generic fused kernel's LDS score row
def test_generic_fused_kernel_with_a_score_row_beyond_64_kib():
    """attention_decode_fused_kernel<0> sizes its LDS score row by max_seq: head size 80 with max_seq 20000 asks for 80 KiB, the opt-in path, at
    position 100; max_seq 41000 asks for more than 160 KiB and is refused (NTK_E_SHAPE) before any launch, output and caches unchanged."""
    nh, nkv, hd, pos = 6, 3, 80, 100
    row = nkv * hd
    lds = lambda max_seq: 4 * (3 * hd + 16 + 4 * hd + max_seq + 1)          # attn_lds(hd, max_seq, 3), csrc/attention.hip
    assert 64 * 1024 < lds(20000) <= 160 * 1024 < lds(41000)
    r = np.random.default_rng(80)
    q = r.standard_normal(nh * hd).astype(np.float32)
    k = r.standard_normal(row).astype(np.float32)
    v = r.standard_normal(row).astype(np.float32)
    for max_seq in (20000, 41000):
        kc, vc = _junk(max_seq * row, 80).copy(), _junk(max_seq * row, 81).copy()
        kc[: pos * row] = _halves(pos * row, 80)
        vc[: pos * row] = _halves(pos * row, 81)
        if max_seq == 20000:
            ref, kc_ref, vc_ref = oracle_step(q, k, v, kc, vc, pos, nh, nkv, hd, max_seq)
            got = launch_step("fused", q, k, v, kc, vc, pos, nh, nkv, hd, max_seq)
            check_step("fused, 80 KiB score row", got, ref, kc_ref, vc_ref, kc, vc, pos, nkv, hd, max_seq)
            continue
        kcd, vcd = Cache(kc), Cache(vc)
        od = DB.from_numpy(np.full(nh * hd, -7.5, np.float32))
        with pytest.raises(_lib.NtkError) as e:
            ops.attention_decode_fused(od, DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v), kcd.ptr, vcd.ptr, DB.from_numpy(np.array([pos], np.int32)),
                                       nh, nkv, hd, max_seq, float(1 / np.sqrt(hd)), THETA)
        assert e.value.status == E_SHAPE
        ops.synchronize()
        assert (od.numpy() == -7.5).all() and np.array_equal(kcd.read(), kc) and np.array_equal(vcd.read(), vc)


# ------------------------------------------------------------------------------------------------ the prompt kernels
def prefill_case(r, T, start, nh, nkv, hd, max_seq, amp=1.0):
    row = nkv * hd
    salt = int(r.integers(0, 1 << 20))
    kc, vc = _junk(max_seq * row, salt).copy(), _junk(max_seq * row, salt + 1).copy()
    live = (start + T) * row
    kc[:live] = _halves(live, salt)
    vc[:live] = _halves(live, salt + 1)
    Q = (r.standard_normal(T * nh * hd) * amp).astype(np.float32)
    return Q, kc, vc


def prefill_against_oracle(form, Q, kc, vc, T, start, nh, nkv, hd, max_seq, what, shift=0):
    scale = float(1 / np.sqrt(hd))
    ref = O.attention_prefill(Q, kc, vc, T, start, nh, nkv, hd, max_seq, scale)
    kcd, vcd = Cache(kc, shift), Cache(vc, shift)
    od = DB.from_numpy(np.full(T * nh * hd, np.nan, np.float32))
    ops.launch_attention_prefill(od, DB.from_numpy(Q), kcd.ptr, vcd.ptr, T, start, nh, nkv, hd, max_seq, scale)
    got = od.numpy()
    assert np.isfinite(got).all(), what
    amp = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    note(form, hd, err / amp, 2e-5)
    assert err <= 2e-5 * amp, (what, err)                                      # test_attention_prefill_mfma_random_sweep's bar
    assert np.array_equal(kcd.read(), kc) and np.array_equal(vcd.read(), vc), what


def test_attention_prefill_tiled_random_sweep_at_64_and_256():
    """40 random (tokens, start, head counts, Q amplitude) launches of attention_prefill_tiled_kernel<8> and <32> (the 96 KiB one): full, diagonal
    and ragged 64-key tiles, 32-query tiles with and without live queries, prefixes that end inside a tile, junk behind the last key"""
    r = np.random.default_rng(6425640)
    for case in range(40):
        hd = (64, 256)[case % 2]
        nkv = int(r.choice([1, 2, 4])); nh = nkv * int(r.choice([1, 2, 4]))
        T = int(r.choice([1, 2, 31, 32, 33, 63, 64, 65, 97, 200]))
        start = int(r.choice([0, 1, 31, 32, 63, 64, 65, 257]))
        max_seq = start + T + int(r.integers(0, 70))
        amp = float(r.choice([0.1, 1.0, 6.0]))
        Q, kc, vc = prefill_case(r, T, start, nh, nkv, hd, max_seq, amp)
        prefill_against_oracle("ntk_attention_prefill, tiled, random sweep", Q, kc, vc, T, start, nh, nkv, hd, max_seq, (case, hd, T, start, nh, nkv, amp))


@pytest.mark.parametrize("T", [2, 9, 40])
@pytest.mark.parametrize("geom", ANY, ids=gid)
def test_attention_prefill_generic_kernel_with_several_queries(geom, T):
    """attention_kernel<0>, causal, more than one query: a prompt at head size 80 / 96, or at 128 on unaligned caches; starts 0 and 130"""
    nh, nkv, hd, shift = geom
    r = np.random.default_rng(1000 * hd + T)
    for start in (0, 130):
        max_seq = start + T + 29
        Q, kc, vc = prefill_case(r, T, start, nh, nkv, hd, max_seq)
        prefill_against_oracle("ntk_attention_prefill, generic, T > 1", Q, kc, vc, T, start, nh, nkv, hd, max_seq, (geom, T, start), shift)


def test_attention_prefill_tiled_256_behind_a_long_prefix():
    """head size 256, 33 queries (a ragged second query tile) behind 1000 keys"""
    nh, nkv, hd, T, start = 8, 2, 256, 33, 1000
    r = np.random.default_rng(2561000)
    Q, kc, vc = prefill_case(r, T, start, nh, nkv, hd, start + T + 40)
    prefill_against_oracle("ntk_attention_prefill, tiled, start 1000", Q, kc, vc, T, start, nh, nkv, hd, start + T + 40, (T, start))


@pytest.mark.parametrize("hd", [64, 256])
def test_attention_prefill_segments_mixed_list_against_the_oracle(hd):
    """test_attention_segments_gpu.py's mixed segment list (lengths 1 .. 70 around the 16- and 64-row borders, the end of the context) at head sizes 64
    and 256: every segment within 2e-5 of the ORACLE's attention_prefill on that segment, and the bits of ntk_attention_prefill on it alone"""
    segments = SEG.SET_A
    Q, caches = SEG.inputs("A", hd)
    got, tail = SEG.run_segments(Q, segments, caches, hd)
    assert np.array_equal(tail, np.full(tail.shape, SEG.SENTINEL))
    alone = SEG.single(Q, segments, caches, hd)
    row = 0
    for s, (n, start) in enumerate(segments):
        assert np.isfinite(got[s]).all(), (s, n, start)
        assert np.array_equal(got[s].view(np.uint32), alone[s].view(np.uint32)), (s, n, start)
        ref = O.attention_prefill(Q[row:row + n].reshape(-1), caches[s][0], caches[s][1], n, start, SEG.NH, SEG.NKV, hd, SEG.MAX_SEQ, float(1 / np.sqrt(hd)))
        err = float(np.abs(got[s].reshape(-1) - ref).max())
        note("ntk_attention_prefill_segments against the oracle", hd, err, 2e-5)
        assert err <= 2e-5, (s, n, start, err)
        row += n
