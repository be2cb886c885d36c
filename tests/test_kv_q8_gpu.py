"""The 8-bit (Q8_0) KV cache on the GPU: the store kernels bit for bit against the numpy quantiser, the decode attention against a float64
attention over the EXACTLY dequantised cache at the F16 kernels' own bar (3e-5), the dequantiser bit for bit, and the engine option.

Run on the MI355X box:  python -m pytest tests/test_kv_q8_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from ntransformer_amd import _lib, kv_q8, ops
from ntransformer_amd import engine as E
from ntransformer_amd.kv_q8 import Q8Cache
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O

pytestmark = pytest.mark.gpu
THETA = 500000.0


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261017, seed]))


def random_blocks(r, n, nb):
    """n rows of nb canonical blocks with UNIT-VARIANCE values, like the N(0, 1) rows of test_hip_kernels.make_cache: the 3e-5 bar of the decode tests is
    absolute and is the F16 kernels' bar on such rows, so it means the same thing only on data of the same scale.  Quants uniform in [-127, 127]
    (variance 127 * 128 / 3 = 73.3^2), scales uniform in [0.5, 1.4] / 73.3 (mean square 0.97 / 73.3^2)."""
    d = (r.uniform(0.5, 1.4, (n, nb)) / 73.3).astype(np.float16)
    q = r.integers(-127, 128, (n, nb, 32)).astype(np.int8)
    return kv_q8.to_blocks(d, q)


def regime_splits(pos):
    return 4 if pos < 544 else 16 if pos < 3072 else 32   # Model::kv_q8_splits(Model::attention_regime(pos, 128))


# ------------------------------------------------------------------------------------------------ quantiser and store
def store_inputs(r, T, per, kind):
    k = r.standard_normal((T, per)).astype(np.float32)
    v = (r.standard_normal((T, per)) * 3).astype(np.float32)
    if kind == "ties":      # amax = 127 -> d = 1, id = 1: x * id = k + 0.5 exactly
        k = (r.integers(-126, 126, (T, per)) + 0.5).astype(np.float32); k[:, ::32] = 127.0
        v = (r.integers(-60, 60, (T, per)) + 0.5).astype(np.float32) * 2; v[:, 5::32] = -254.0   # d = 2, id = 0.5
    elif kind == "zeros":   # zero blocks, subnormal amax, a lone tiny normal
        k[:, :64] = 0.0; k[:, 64:96] = 0.0; k[:, 70] = 1e-40; k[:, 96:128] = 0.0; k[:, 100] = -3e-39
        v[:, :32] = 0.0; v[:, 32:64] = 0.0; v[:, 40] = 1.5e-38
    return k, v


@pytest.mark.parametrize("T,start", [(1, 0), (3, 5), (64, 17), (1024, 1000)])
@pytest.mark.parametrize("kind", ["normal", "ties", "zeros"])
def test_kv_store_q8_is_bit_exact_against_the_numpy_quantiser(T, start, kind):
    nkv, hd, max_seq = 2, 128, 2048
    per = nkv * hd
    r = rng(T * 3 + start + len(kind))
    k, v = store_inputs(r, T, per, kind)
    kc, vc = Q8Cache(max_seq, nkv, hd, fill=0x5A), Q8Cache(max_seq, nkv, hd, fill=0xA5)
    before_k, before_v = kc.raw(), vc.raw()
    kv_q8.kv_store_q8(kc, vc, DB.from_numpy(k), DB.from_numpy(v), T, nkv, hd, start)
    for cache, x, before in ((kc, k, before_k), (vc, v, before_v)):
        want = kv_q8.to_blocks(*kv_q8.quantize_q8_0(x))
        assert np.array_equal(cache.read_blocks(start, T), want)
        after = cache.raw()
        qmask = np.ones(after.size, bool)
        qmask[start * per:(start + T) * per] = False
        s0 = max_seq * per + start * (per // 32) * 2
        qmask[s0:s0 + T * (per // 32) * 2] = False
        assert np.array_equal(after[qmask], before[qmask])   # rows outside the range untouched


def test_kv_store_q8_drops_rows_past_the_cache_end():
    nkv, hd, max_seq, T = 2, 128, 64, 4
    r = rng(99)
    k, v = store_inputs(r, T, nkv * hd, "normal")
    kc, vc = Q8Cache(max_seq, nkv, hd), Q8Cache(max_seq, nkv, hd)
    kv_q8.kv_store_q8(kc, vc, DB.from_numpy(k), DB.from_numpy(v), T, nkv, hd, max_seq - 2)
    assert np.array_equal(kc.read_blocks(max_seq - 2, 2), kv_q8.to_blocks(*kv_q8.quantize_q8_0(k[:2])))


@pytest.mark.parametrize("T,start,nh,nkv", [(4, 0, 8, 2), (64, 100, 32, 8), (1024, 1024, 8, 2), (37, 3, 16, 1)])
def test_rope_kv_store_q8_equals_rope_then_store(T, start, nh, nkv):
    hd, max_seq = 128, 2048
    r = rng(T + start + nh)
    q = r.standard_normal((T, nh * hd)).astype(np.float32)
    k = r.standard_normal((T, nkv * hd)).astype(np.float32)
    v = r.standard_normal((T, nkv * hd)).astype(np.float32)
    pos = DB.from_numpy(np.arange(start, start + T, dtype=np.int32))
    qa, ka, va = DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v)
    kca, vca = Q8Cache(max_seq, nkv, hd), Q8Cache(max_seq, nkv, hd)
    ops.launch_rope(qa, ka, pos, 1, T, nh, nkv, hd, THETA, 1.0, 0)
    kv_q8.kv_store_q8(kca, vca, ka, va, T, nkv, hd, start)
    qb, kb = DB.from_numpy(q), DB.from_numpy(k)
    kcb, vcb = Q8Cache(max_seq, nkv, hd), Q8Cache(max_seq, nkv, hd)
    kv_q8.rope_kv_store_q8(qb, kb, va, pos, T, nh, nkv, hd, THETA, kcb, vcb, start)
    assert np.array_equal(qa.numpy(), qb.numpy())
    assert np.array_equal(kb.numpy(), k.reshape(-1))                     # k is only read
    assert np.array_equal(kca.raw(), kcb.raw()) and np.array_equal(vca.raw(), vcb.raw())
    assert kca.read_blocks(start, T).any()


@pytest.mark.parametrize("n", [1, 33, 1500])
def test_kv_dequant_q8_f16_is_bit_exact(n):
    nkv, hd, max_seq = 2, 128, 2048
    r = rng(n)
    kb, vb = random_blocks(r, n, nkv * hd // 32), random_blocks(r, n, nkv * hd // 32)
    kb[0, 0, :2] = np.array([65504.0], np.float16).view(np.uint8)        # overflow to inf in half, as the formula says
    kc, vc = Q8Cache(max_seq, nkv, hd), Q8Cache(max_seq, nkv, hd)
    kc.write_blocks(0, kb); vc.write_blocks(0, vb)
    k16, v16 = DB.from_numpy(np.full(n * nkv * hd, 0x1234, np.uint16)), DB.from_numpy(np.full(n * nkv * hd, 0x1234, np.uint16))
    kv_q8.kv_dequant_q8_f16(k16, v16, kc, vc, n, nkv, hd)
    assert np.array_equal(k16.numpy(np.uint16), kv_q8.dequantize_f16(kb).reshape(-1))
    assert np.array_equal(v16.numpy(np.uint16), kv_q8.dequantize_f16(vb).reshape(-1))


# ------------------------------------------------------------------------------------------------ decode attention
def run_decode(r, pos, nh, nkv, nsplit, max_seq=None, junk=False, launches=1):
    hd = 128
    max_seq = max_seq or max(pos + 1, 64)
    nb = nkv * hd // 32
    kb, vb = random_blocks(r, pos, nb), random_blocks(r, pos, nb)
    q = r.standard_normal(nh * hd).astype(np.float32)
    k = r.standard_normal(nkv * hd).astype(np.float32)
    v = r.standard_normal(nkv * hd).astype(np.float32)
    kc, vc = Q8Cache(max_seq, nkv, hd), Q8Cache(max_seq, nkv, hd)
    if junk:   # rows from the position on: NaN / inf scale patterns, 0x80 quants
        pat = np.array([0x7E00, 0xFE00, 0x7C00, 0xFC00, 0x7BFF, 0xFFFF], np.uint16)
        for c in (kc, vc):
            jd = pat[r.integers(0, len(pat), (max_seq - pos, nb))].view(np.float16)
            c.write_blocks(pos, kv_q8.to_blocks(jd, np.full((max_seq - pos, nb, 32), -128, np.int8)))
    if pos:
        kc.write_blocks(0, kb); vc.write_blocks(0, vb)
    od = DB.from_numpy(np.full(nh * hd, np.nan, np.float32))
    kv_q8.attention_decode_q8(od, DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v), kc, vc, DB.from_numpy(np.array([pos], np.int32)),
                              nh, nkv, hd, max_seq, float(1 / np.sqrt(hd)), THETA, nsplit, launches=launches)
    return dict(out=od.numpy(), q=q, k=k, v=v, kb=kb, vb=vb, kc=kc, vc=vc, max_seq=max_seq)


def check_decode(pos, nh, nkv, nsplit):
    hd = 128
    r = rng(pos * 7 + nh * 3 + nsplit)
    g = run_decode(r, pos, nh, nkv, nsplit)
    out = g["out"]
    assert np.isfinite(out).all()
    # the new row, read back: V bit-exact; K within one quantisation step of the numpy quantiser of the oracle's rotation (device vs glibc sin / cos)
    new_k, new_v = g["kc"].read_blocks(pos, 1), g["vc"].read_blocks(pos, 1)
    rq, rk = O.rope(g["q"], g["k"], [pos], nh, nkv, hd, THETA)
    assert np.array_equal(new_v, kv_q8.to_blocks(*kv_q8.quantize_q8_0(g["v"][None, :])))
    wd, wq = kv_q8.quantize_q8_0(rk[None, :])
    gd, gq = kv_q8.from_blocks(new_k)
    assert np.abs(gq.astype(np.int32) - wq.astype(np.int32)).max() <= 1
    assert np.abs(gd.astype(np.float32) - wd.astype(np.float32)).max() <= 2.0 ** -10 * float(wd.max())
    if pos:   # earlier rows untouched
        assert np.array_equal(g["kc"].read_blocks(0, pos), g["kb"]) and np.array_equal(g["vc"].read_blocks(0, pos), g["vb"])
    K = np.concatenate([kv_q8.dequantize_exact(g["kb"]), kv_q8.dequantize_exact(new_k)]).reshape(pos + 1, nkv * hd)
    V = np.concatenate([kv_q8.dequantize_exact(g["vb"]), kv_q8.dequantize_exact(new_v)]).reshape(pos + 1, nkv * hd)
    # q as the DEVICE rotated it is not observable; the oracle's rotation differs in the last bit of sin / cos: far inside the bar
    ref = kv_q8.attention_f64(rq, K, V, nh, nkv, hd, float(1 / np.sqrt(hd)))
    err = float(np.abs(out - ref).max())
    print("pos %d nh %d nkv %d nsplit %d: |out - f64| = %.3g" % (pos, nh, nkv, nsplit, err))
    assert err <= 3e-5, err


@pytest.mark.parametrize("pos,nh,nkv,nsplit", [(8191, 8, 2, 32), (1500, 16, 2, 16)])
def test_attention_decode_q8_small_amplitude_v_under_peaked_scores(pos, nh, nkv, nsplit):
    """V of amplitude 1e-2 (scales d ~ 1e-4) under peaked scores (q x 3: most softmax weights are far below the maximum).  The V scale enters as an exact
    mantissa (into P) times an exact power of two (onto the quants), so small weights x small scales lose nothing to the F16 subnormals.  The kernel's
    arithmetic is homogeneous in the scale of V, so the bar is the unit-scale bar times the amplitude: 3e-5 x 1e-2."""
    hd, amp = 128, 1e-2
    r = rng(pos + nh + 77)
    nb = nkv * hd // 32
    kb, vb = random_blocks(r, pos, nb), random_blocks(r, pos, nb)
    vd, vq = kv_q8.from_blocks(vb)
    vb = kv_q8.to_blocks((vd.astype(np.float32) * amp).astype(np.float16), vq)
    q = (r.standard_normal(nh * hd) * 3).astype(np.float32)
    k = r.standard_normal(nkv * hd).astype(np.float32)
    v = (r.standard_normal(nkv * hd) * amp).astype(np.float32)
    max_seq = pos + 1
    kc, vc = Q8Cache(max_seq, nkv, hd), Q8Cache(max_seq, nkv, hd)
    kc.write_blocks(0, kb); vc.write_blocks(0, vb)
    od = DB.from_numpy(np.full(nh * hd, np.nan, np.float32))
    kv_q8.attention_decode_q8(od, DB.from_numpy(q), DB.from_numpy(k), DB.from_numpy(v), kc, vc, DB.from_numpy(np.array([pos], np.int32)),
                              nh, nkv, hd, max_seq, float(1 / np.sqrt(hd)), THETA, nsplit)
    rq, _ = O.rope(q, k, [pos], nh, nkv, hd, THETA)
    K = np.concatenate([kv_q8.dequantize_exact(kb), kv_q8.dequantize_exact(kc.read_blocks(pos, 1))]).reshape(pos + 1, nkv * hd)
    V = np.concatenate([kv_q8.dequantize_exact(vb), kv_q8.dequantize_exact(vc.read_blocks(pos, 1))]).reshape(pos + 1, nkv * hd)
    ref = kv_q8.attention_f64(rq, K, V, nh, nkv, hd, float(1 / np.sqrt(hd)))
    err = float(np.abs(od.numpy() - ref).max())
    print("pos %d nh %d: |out - f64| = %.3g (bar %.3g, |ref| max %.3g)" % (pos, nh, err, 3e-5 * amp, float(np.abs(ref).max())))
    assert err <= 3e-5 * amp, err


DECODE_CASES = []
for _pos in (0, 3, 31, 32, 607, 1500, 3071, 4095, 8191, 32767, 131071):
    _s = regime_splits(_pos)
    _splits = [_s, 2 * _s + 3] + ([_pos + 6] if _pos <= 32 else []) + ([1] if _pos in (607, 4095) else [])
    for _nh, _nkv in ((8, 2), (16, 2)):   # GQA 4 and 8
        for _n in _splits:
            DECODE_CASES.append((_pos, _nh, _nkv, _n))
DECODE_CASES += [(1500, 3, 3, 16), (3071, 10, 2, 16), (4095, 16, 1, 32), (33, 5, 1, 4)]   # 1 / 5 / 16 query heads per KV head


@pytest.mark.parametrize("pos,nh,nkv,nsplit", DECODE_CASES)
def test_attention_decode_q8_equals_float64_attention_over_the_exact_cache(pos, nh, nkv, nsplit):
    check_decode(pos, nh, nkv, nsplit)


@pytest.mark.parametrize("pos", [5, 40, 607, 1500, 3100])
@pytest.mark.parametrize("nh,nkv", [(32, 8), (64, 8)])
def test_attention_decode_q8_ignores_rows_past_the_position(pos, nh, nkv):
    """Rows from the position on hold NaN / inf scale bit patterns and 0x80 quants: the output and the cache rows up to the position are the
    bits of a run over a zeroed tail (the kernel masks by selects)."""
    nsplit = regime_splits(pos)
    a = run_decode(rng(pos + nh), pos, nh, nkv, nsplit, max_seq=4096)
    b = run_decode(rng(pos + nh), pos, nh, nkv, nsplit, max_seq=4096, junk=True)
    assert np.isfinite(a["out"]).all()
    assert np.array_equal(a["out"], b["out"])
    for c in ("kc", "vc"):
        assert np.array_equal(a[c].read_blocks(0, pos + 1), b[c].read_blocks(0, pos + 1))
        tail = b[c].read_blocks(pos + 1, 4096 - pos - 1)
        assert (tail[..., 2:] == 0x80).all()                                                       # later rows untouched


@pytest.mark.parametrize("pos,nsplit", [(100, 4), (2000, 16), (9000, 32)])
def test_attention_decode_q8_is_deterministic(pos, nsplit):
    a = run_decode(rng(pos), pos, 32, 8, nsplit)
    b = run_decode(rng(pos), pos, 32, 8, nsplit, launches=2)   # (the second launch re-quantises the same row: same bits)
    assert np.array_equal(a["out"], b["out"])
    assert np.array_equal(a["kc"].raw(), b["kc"].raw()) and np.array_equal(a["vc"].raw(), b["vc"].raw())


@pytest.mark.parametrize("hd", [64, 256])
def test_attention_decode_q8_refuses_other_head_sizes(hd):
    nh, nkv, max_seq = 8, 2, 256
    kc, vc = Q8Cache(max_seq, nkv, hd), Q8Cache(max_seq, nkv, hd)
    z = lambda n: DB.zeros(n)
    st = kv_q8.attention_decode_q8_status(z(nh * hd * 4), z(nh * hd * 4), z(nkv * hd * 4), z(nkv * hd * 4), kc, vc, DB.from_numpy(np.array([7], np.int32)),
                                          nh, nkv, hd, max_seq, 0.1, THETA, 4)
    assert st == -2   # NTK_E_SHAPE
    st = kv_q8.attention_decode_q8_status(z(34 * 128 * 4), z(34 * 128 * 4), z(2 * 128 * 4), z(2 * 128 * 4), Q8Cache(64, 2, 128), Q8Cache(64, 2, 128),
                                          DB.from_numpy(np.array([7], np.int32)), 34, 2, 128, 64, 0.1, THETA, 4)
    assert st == -2   # 17 query heads per KV head


# ------------------------------------------------------------------------------------------------ engine
def tiny128_spec(mix="Q8_0"):
    return E.SynthSpec(256, 512, 2, 2, 1, 512, 4096, 1e-5, THETA, 256, 257, mix.encode(), 20261017)


def small_spec(mix="Q8_0"):
    s = E.synth_spec("small", mix)
    s.ctx = 4096
    return s


def engine(spec, ctx, kv, **opts):
    e = E.Engine()
    e.set_option("synth_threads", 16)
    e.set_option("kv_cache", kv)
    for key, val in opts.items():
        e.set_option(key, val)
    e.load_synthetic(spec, ctx)
    return e


def geometry(spec):
    hd = spec.hidden // spec.heads
    return spec.layers, spec.kv_heads, hd, spec.kv_heads * hd


@pytest.mark.parametrize("make", [tiny128_spec, small_spec])
def test_engine_option_accounting_and_debug_access(make):
    spec, ctx = make(), 1024
    L, nkv, hd, per = geometry(spec)
    f, q = engine(spec, ctx, "f16"), engine(spec, ctx, "q8_0")
    f16_bytes = 2 * L * ctx * per * 2
    assert f.kv_cache_bytes() == f16_bytes
    assert q.kv_cache_bytes() == 2 * L * kv_q8.cache_bytes(ctx, nkv, hd) + 2 * ctx * per * 2     # the 8-bit caches + exactly one layer's F16 image
    assert 2 * L * kv_q8.cache_bytes(ctx, nkv, hd) <= 0.54 * f16_bytes
    for pos in (0, 100, 1000):
        assert f.bytes_per_token(pos) - q.bytes_per_token(pos) == 2 * L * (pos + 2) * (per * 2 - per * 17 // 16)
    with pytest.raises(_lib.NtkError) as ei:
        q.set_option("kv_cache", "f16")                       # after the load
    assert "before" in str(ei.value)
    with pytest.raises(_lib.NtkError) as ei:
        q.kv_read(0, 0, 1, per)
    assert ei.value.status == -1                              # NTK_E_DTYPE
    with pytest.raises(_lib.NtkError) as ei:
        f.kv_read_q8(0, 0, 1, per)
    assert ei.value.status == -1
    r = rng(5)
    kb, vb = random_blocks(r, 7, per // 32), random_blocks(r, 7, per // 32)
    q.kv_write_q8(L - 1, 3, kb, vb)
    gk, gv = q.kv_read_q8(L - 1, 3, 7, per)
    assert np.array_equal(gk, kb) and np.array_equal(gv, vb)
    f.close(); q.close()


def test_engine_refuses_what_the_8_bit_cache_does_not_cover():
    e = E.Engine()
    e.set_option("kv_cache", "q8_0")
    with pytest.raises(_lib.NtkError) as ei:
        e.load_synthetic(E.synth_spec("tiny", "Q8_0"), 256)   # head_dim 64
    assert "head_dim" in str(ei.value)
    e.close()
    e = E.Engine()
    e.set_option("kv_cache", "q8_0")
    e.tp_configure(0, 2)
    with pytest.raises(_lib.NtkError) as ei:
        e.load_synthetic(small_spec(), 256)
    assert "tensor parallelism" in str(ei.value)
    e.close()


def test_engine_cache_contents_after_a_prompt_pass():
    """Layer 0 after a 40-token prompt (the fused RoPE + store launch) and after a 3-token pass (ntk_rope + ntk_kv_store_q8): the cache read with
    debug_kv_read_q8 against the numpy quantiser applied to the EXACT F32 inputs of the store, which the engine leaves aside on request
    (nt_engine_debug_kv_inputs_capture: the layer's k projection before the rotation, and v).  V: block for block, bit-exact.  K: the oracle's rotation
    of the captured k differs from the device's in the last bit of sin / cos, so quants within one step and scales within a half ulp-pair (2^-10)."""
    spec, ctx = small_spec(), 256
    L, nkv, hd, per = geometry(spec)
    nh = spec.heads
    e = engine(spec, ctx, "q8_0")
    e.kv_inputs_capture(0)
    for start, T in ((0, 40), (40, 3)):
        prompt = [int(t) for t in rng(8 + T).integers(0, 2000, T)]
        e.forward(prompt, start)
        k_in, v_in = e.kv_inputs_read(T, per)
        got_k, got_v = e.kv_read_q8(0, start, T, per)
        assert np.abs(v_in).max() > 0
        assert np.array_equal(got_v, kv_q8.to_blocks(*kv_q8.quantize_q8_0(v_in)))
        rk = np.stack([O.rope(np.zeros(nh * hd, np.float32), k_in[t], [start + t], nh, nkv, hd, THETA)[1] for t in range(T)])
        wd, wq = kv_q8.quantize_q8_0(rk)
        gd, gq = kv_q8.from_blocks(got_k)
        assert np.abs(gq.astype(np.int32) - wq.astype(np.int32)).max() <= 1
        assert (np.abs(gd.astype(np.float64) - wd.astype(np.float64)) <= 2.0 ** -10 * wd.astype(np.float64)).all()
        frac = float((gq == wq).mean())
        print("rows %d..%d: %.4f of the K quants equal the numpy quantiser of the oracle's rotation" % (start, start + T, frac))
        assert frac > 0.99
    e.close()


def seed_cache(e, spec, n, seed):
    L, nkv, hd, per = geometry(spec)
    r = rng(seed)
    for layer in range(L):
        e.kv_write_q8(layer, 0, random_blocks(r, n, per // 32), random_blocks(r, n, per // 32))


@pytest.mark.parametrize("make", [tiny128_spec, small_spec])
def test_engine_fused_eager_graph_and_unfused_agree_across_the_regime_borders(make):
    """8 decode steps across each border (544: 4 -> 16 splits, 3072: 16 -> 32) over seeded caches: eager launches and hipGraph replay give the same bits;
    the fused=0 step (8-bit store, dequantise to the F16 image, F16 attention kernel) agrees with the fused step within the launch-mode tolerance 1e-3."""
    spec, ctx = make(), 4096
    e = engine(spec, ctx, "q8_0")
    seed_cache(e, spec, 3080, 11)
    toks = [int(t) for t in rng(12).integers(0, 500, 8)]
    for p0 in (540, 3068):
        eager = [e.decode_fused(t, p0 + i, False) for i, t in enumerate(toks)]
        graph = [e.decode_fused(t, p0 + i, True) for i, t in enumerate(toks)]
        for a, b in zip(eager, graph):
            assert np.isfinite(a).all() and np.array_equal(a, b)
        plain = [e.forward([t], p0 + i) for i, t in enumerate(toks)]
        err = max(float(np.abs(a - b).max()) for a, b in zip(eager, plain))
        print("positions %d..: |fused - unfused| = %.3g" % (p0, err))
        assert err <= 1e-3
    e.close()


def test_engine_prompt_chunk_attends_to_the_earlier_chunk():
    spec, ctx = small_spec(), 2048
    L, nkv, hd, per = geometry(spec)
    e = engine(spec, ctx, "q8_0")
    prompt = [int(t) for t in rng(13).integers(0, 2000, 1030)]
    e.forward(prompt[:1024], 0)
    a = e.forward(prompt[1024:], 1024)
    a2 = e.forward(prompt[1024:], 1024)
    assert np.array_equal(a, a2)
    seed_cache(e, spec, 1024, 14)                            # chunk 0's rows replaced in every layer
    b = e.forward(prompt[1024:], 1024)
    assert np.isfinite(b).all() and float(np.abs(a - b).max()) > 1e-2
    e.close()


def test_shared_weights_one_f16_and_one_q8_sequence():
    spec, ctx, n = small_spec(), 512, 12
    prompts = [[int(t) for t in rng(15).integers(0, 2000, 33)], [int(t) for t in rng(16).integers(0, 2000, 21)]]
    kinds = ("f16", "q8_0")
    solo = []
    for pr, kv in zip(prompts, kinds):
        e = engine(spec, ctx, kv)
        lg = e.forward(pr, 0)
        toks = e.decode_greedy_steps(int(np.argmax(lg)), len(pr), n)
        solo.append((lg, toks, e.decode_fused(toks[-1], len(pr) + n, True)))
        e.close()
    a = engine(spec, ctx, "f16")
    b = E.Engine()
    b.set_option("kv_cache", "q8_0")
    b.load_shared(a, ctx)
    assert b.kv_cache_bytes() < a.kv_cache_bytes()
    for rep in range(2):
        for i, eng in enumerate((a, b)):
            lg = eng.forward(prompts[i], 0)
            toks = eng.decode_greedy_steps(int(np.argmax(lg)), len(prompts[i]), n)
            assert np.array_equal(lg, solo[i][0]) and toks == solo[i][1], (rep, i)
            assert np.array_equal(eng.decode_fused(toks[-1], len(prompts[i]) + n, True), solo[i][2]), (rep, i)
    b.close(); a.close()
