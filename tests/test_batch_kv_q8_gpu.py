"""The batched decode step over the 8-bit (Q8_0) KV cache, behind the "batch_kv_q8" option: per-slot 8-bit caches, seq_forward into a slot, the
batched quantising store, the batched step against the solo fused step, independence of companions / order / slot numbers, and generation.

Bars.  Bit equality wherever the same code runs on the same inputs (seq_forward vs forward; a row under different companions).  The new cache row
against the numpy quantiser of the store's captured F32 inputs at test_kv_q8_gpu.test_engine_cache_contents_after_a_prompt_pass's bars (V blocks
bit-exact, K quants within one step, K scales within 2^-10).  A batched row against its solo nt_engine_decode_fused run: 1e-3, the header's contract
(include/ntransformer.h), asserted for rows at positions >= 512; rows below are printed only -- the two paths feed slightly different F32 k / v into
the quantiser (prompt-pass projections vs decode GEMV), one quant of the NEW row may flip, and that row's softmax weight is not small at short
contexts; the kernel test (test_attention_q8_batch_gpu.py) and the store test here cover those rows exactly.  One GPU run's deviations:
profiles/batch_kv_q8_parity.txt.

Run on the MI355X box:  python -m pytest tests/test_batch_kv_q8_gpu.py -m gpu -x -q -s"""
import numpy as np
import pytest

from ntransformer_amd import _lib, kv_q8
from ntransformer_amd import engine as E
from oracle import oracle as O

pytestmark = pytest.mark.gpu
THETA = 500000.0
CTX = 4096
_pool = {}


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261019, seed]))


def tiny128_spec(mix="Q8_0"):   # (tests/test_kv_q8_gpu.py's, restated)
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


def blocks(n, nb, salt):
    """rows [0, n) of a stream of canonical blocks named by `salt` (unit-variance values: test_kv_q8_gpu.random_blocks); a window of pools drawn once,
    so a shorter request is a prefix of a longer one"""
    if "q" not in _pool:
        r = rng(1)
        _pool["q"] = r.integers(-127, 128, 1 << 22).astype(np.int8)
        _pool["d"] = (r.uniform(0.5, 1.4, 1 << 18) / 73.3).astype(np.float16)
    q, d = _pool["q"], _pool["d"]
    qo, do = (salt * 104729) % (q.size - 1), (salt * 7919) % (d.size - 1)
    return kv_q8.to_blocks(np.resize(np.roll(d, -do), n * nb).reshape(n, nb), np.resize(np.roll(q, -qo), n * nb * 32).reshape(n, nb, 32))


def stream_blocks(stream, layer, n, nb):
    """(K, V) rows [0, n) of cache content `stream` in `layer`"""
    return blocks(n, nb, 1 + 64 * stream + 2 * layer), blocks(n, nb, 2 + 64 * stream + 2 * layer)


def seed_slot(e, spec, slot, stream, n, pos0=0):
    """rows [pos0, n) of every layer of `slot` <- content `stream` (slot None: the solo engine's cache)"""
    L, nkv, hd, per = geometry(spec)
    for layer in range(L):
        kb, vb = stream_blocks(stream, layer, n, per // 32)
        if slot is None:
            e.kv_write_q8(layer, pos0, kb[pos0:], vb[pos0:])
        else:
            e.kv_write_q8_slot(slot, layer, pos0, kb[pos0:], vb[pos0:])


def whole_cache(e, spec, slot):
    L, nkv, hd, per = geometry(spec)
    return [e.kv_read_q8_slot(slot, layer, 0, e.max_context, per) for layer in range(L)]


def same_cache(a, b):
    return all(np.array_equal(ka, kb) and np.array_equal(va, vb) for (ka, va), (kb, vb) in zip(a, b))


# ------------------------------------------------------------------------------------------------ 1. option, accounting, debug access
def test_option_accounting_and_debug_access():
    spec, ctx, N = small_spec(), 256, 3
    L, nkv, hd, per = geometry(spec)
    e = E.Engine()
    e.set_option("kv_cache", "q8_0")
    e.set_option("sequences", 2)
    with pytest.raises(_lib.NtkError) as ei:                     # without the option: the refusal as it was
        e.load_synthetic(spec, ctx)
    assert ei.value.status == -2 and "sequences" in str(ei.value)
    e.close()
    q = engine(spec, ctx, "q8_0", batch_kv_q8=1, sequences=N)
    assert q.kv_cache_bytes() == N * 2 * L * kv_q8.cache_bytes(ctx, nkv, hd) + 2 * ctx * per * 2   # the slots' 8-bit caches + ONE one-layer F16 image
    with pytest.raises(_lib.NtkError) as ei:
        q.set_option("batch_kv_q8", 0)                            # after the load
    assert ei.value.status == -2 and "before" in str(ei.value)
    kb, vb = blocks(7, per // 32, 901), blocks(7, per // 32, 902)
    q.kv_write_q8_slot(N - 1, L - 1, 3, kb, vb)
    gk, gv = q.kv_read_q8_slot(N - 1, L - 1, 3, 7, per)
    assert np.array_equal(gk, kb) and np.array_equal(gv, vb)
    for slot in range(N - 1):                                     # the other slots: still the zeros of the load
        zk, zv = q.kv_read_q8_slot(slot, L - 1, 0, ctx, per)
        assert not zk.any() and not zv.any()
    q.kv_write_q8(0, 5, kb, vb)                                   # slot 0 is the cache the slot-less calls use
    gk, gv = q.kv_read_q8_slot(0, 0, 5, 7, per)
    assert np.array_equal(gk, kb) and np.array_equal(gv, vb)
    for slot in (N, -1, 16):
        with pytest.raises(_lib.NtkError) as ei:
            q.kv_read_q8_slot(slot, 0, 0, 1, per)
        assert ei.value.status == -2                              # NTK_E_SHAPE
        with pytest.raises(_lib.NtkError) as ei:
            q.kv_write_q8_slot(slot, 0, 0, kb[:1], vb[:1])
        assert ei.value.status == -2
    with pytest.raises(_lib.NtkError) as ei:
        q.kv_read_slot(1, 0, 0, 1, per)                           # the F16 pair on this engine
    assert ei.value.status == -1                                  # NTK_E_DTYPE
    q.close()
    f = engine(spec, ctx, "f16", batch_kv_q8=1, sequences=2)      # with the F16 cache the option changes nothing
    assert f.kv_cache_bytes() == 2 * 2 * L * ctx * per * 2
    with pytest.raises(_lib.NtkError) as ei:
        f.kv_read_q8_slot(1, 0, 0, 1, per)
    assert ei.value.status == -1
    with pytest.raises(_lib.NtkError) as ei:
        f.kv_write_q8_slot(1, 0, 0, kb[:1], vb[:1])
    assert ei.value.status == -1
    f.close()


# ------------------------------------------------------------------------------------------------ 2. seq_forward into a slot
def test_seq_forward_into_a_slot_equals_forward_on_a_solo_engine():
    """A 40-token chunk (the fused RoPE + store launch), another slot's prefill in between (the one-layer F16 image is shared: it must carry nothing
    across passes), then a 3-token chunk (ntk_rope + ntk_kv_store_q8): logits and every layer's cache blocks are forward()'s on a fresh solo engine."""
    spec, ctx, s = small_spec(), 256, 2
    L, nkv, hd, per = geometry(spec)
    e, solo = engine(spec, ctx, "q8_0", batch_kv_q8=1, sequences=3), engine(spec, ctx, "q8_0")
    r = rng(21)
    p40, other, p3 = ([int(t) for t in r.integers(0, 2000, n)] for n in (40, 57, 3))
    assert np.array_equal(e.seq_forward(s, p40, 0), solo.forward(p40, 0))
    e.seq_forward(1, other, 0)
    a, b = e.seq_forward(s, p3, 40), solo.forward(p3, 40)
    assert np.isfinite(a).all() and np.array_equal(a, b)
    for layer in range(L):
        gk, gv = e.kv_read_q8_slot(s, layer, 0, ctx, per)
        wk, wv = solo.kv_read_q8(layer, 0, ctx, per)
        assert gk[:43].any() and np.array_equal(gk, wk) and np.array_equal(gv, wv), layer
        zk, zv = e.kv_read_q8_slot(0, layer, 0, ctx, per)         # slot 0 took no part
        assert not zk.any() and not zv.any()
    e.close(); solo.close()


# ------------------------------------------------------------------------------------------------ the 16-slot engines of tests 3 - 5
@pytest.fixture(scope="module", params=["tiny128", "small"])
def rig(request):
    """a 16-slot q8_0 engine at 4096 positions, every slot seeded with its own content stream over the whole context, and a solo q8_0 engine"""
    spec = tiny128_spec() if request.param == "tiny128" else small_spec()
    e = engine(spec, CTX, "q8_0", batch_kv_q8=1, sequences=16)
    solo = engine(spec, CTX, "q8_0")
    for slot in range(16):
        seed_slot(e, spec, slot, slot, CTX)
    yield request.param, spec, e, solo
    e.close(); solo.close()


def restore(e, spec, slots, positions, streams=None):
    """the rows a step wrote <- their seeded content"""
    L, nkv, hd, per = geometry(spec)
    for b, (slot, pos) in enumerate(zip(slots, positions)):
        for layer in range(L):
            kb, vb = stream_blocks(slot if streams is None else streams[b], layer, pos + 1, per // 32)
            e.kv_write_q8_slot(slot, layer, pos, kb[pos:], vb[pos:])


# ------------------------------------------------------------------------------------------------ 3. the batched store is the quantiser
def test_the_batched_store_is_the_quantiser(rig):
    name, spec, e, solo = rig
    L, nkv, hd, per = geometry(spec)
    nh = spec.heads
    positions = [0, 31, 32, 543, 544, 3071, 3072, CTX - 1, 1, 33, 100, 1000, 2000, 3000, 4000, 17]
    slots = [(7 * i + 3) % 16 for i in range(16)]
    tokens = [int(t) for t in rng(31).integers(0, 500, 16)]
    e.kv_inputs_capture(0)
    e.decode_batch(slots, tokens, positions)
    k_in, v_in = e.kv_inputs_read(16, per)
    e.kv_inputs_capture(-1)
    assert np.abs(v_in).max() > 0
    equal = 0.0
    for b, (slot, pos) in enumerate(zip(slots, positions)):
        got_k, got_v = e.kv_read_q8_slot(slot, 0, pos, 1, per)
        assert np.array_equal(got_v, kv_q8.to_blocks(*kv_q8.quantize_q8_0(v_in[b][None, :]))), (b, pos)
        rk = O.rope(np.zeros(nh * hd, np.float32), k_in[b], [pos], nh, nkv, hd, THETA)[1]
        wd, wq = kv_q8.quantize_q8_0(rk[None, :])
        gd, gq = kv_q8.from_blocks(got_k)
        assert np.abs(gq.astype(np.int32) - wq.astype(np.int32)).max() <= 1, (b, pos)
        assert (np.abs(gd.astype(np.float64) - wd.astype(np.float64)) <= 2.0 ** -10 * wd.astype(np.float64)).all(), (b, pos)
        equal += float((gq == wq).mean()) / 16
        # its neighbours keep their seeded content
        lo, hi = max(pos - 1, 0), min(pos + 2, CTX)
        nk, nv = e.kv_read_q8_slot(slot, 0, lo, hi - lo, per)
        wk, wv = stream_blocks(slot, 0, hi, per // 32)
        keep = [i for i in range(lo, hi) if i != pos]
        assert np.array_equal(nk[[i - lo for i in keep]], wk[keep]) and np.array_equal(nv[[i - lo for i in keep]], wv[keep]), (b, pos)
    print("%s: %.4f of the new rows' K quants equal the numpy quantiser of the oracle's rotation" % (name, equal))
    assert equal > 0.99
    restore(e, spec, slots, positions)


# ------------------------------------------------------------------------------------------------ 4. the batched step against the solo step
BATCHES = {   # by the batch's largest position, which picks the split count: 4 below 544, 16 below 3072, 32 from there
    "max543": [543, 0, 31, 32, 512, 542, 100, 1],
    "max544": [544, 543, 0, 520, 33, 15],
    "max3071": [3071, 544, 543, 2000, 0, 1023],
    "max3072": [3072, 3071, 600, 0],
    "max4095": [4095, 0, 543, 544, 3071, 3072, 512, 1024, 2048, 4000, 31, 32, 33, 1, 700, 3500],
}


@pytest.mark.parametrize("batch", list(BATCHES))
def test_a_batched_row_equals_its_solo_fused_step(rig, batch):
    name, spec, e, solo = rig
    positions = BATCHES[batch]
    B = len(positions)
    slots = [(5 * i + 2) % 16 for i in range(B)]
    tokens = [int(t) for t in rng(41 + B).integers(0, 500, B)]
    lg, nxt = e.decode_batch(slots, tokens, positions)
    assert np.isfinite(lg).all()
    restore(e, spec, slots, positions)
    worst = 0.0
    for b, (slot, pos) in enumerate(zip(slots, positions)):
        seed_slot(solo, spec, None, slot, pos)
        ref = solo.decode_fused(tokens[b], pos, False)
        err = float(np.abs(lg[b] - ref).max())
        print("%s %s row %2d slot %2d pos %4d: |batched - solo| = %.3g%s" % (name, batch, b, slot, pos, err, "" if pos >= 512 else "   (not asserted: below 512)"))
        if pos >= 512:
            worst = max(worst, err)
            assert err <= 1e-3, (b, pos, err)
            assert nxt[b] == int(np.argmax(lg[b]))
    print("%s %s: worst asserted deviation %.3g" % (name, batch, worst))


# ------------------------------------------------------------------------------------------------ 5. companions, order and slots do not matter
def test_companions_order_and_slot_numbers_do_not_matter(rig):
    """(The attention's split count follows the batch's LARGEST position -- 4 / 16 / 32 with the borders at 544 and 3072, as the F16 step's form does --
    so the three batches stay inside one regime: the largest position is the row's own, or a companion's below 3072.)"""
    name, spec, e, solo = rig
    X, A, Bc = (123, 1500), (77, 9), (301, 2900)          # (token, position): the row under test and two companions
    for slot in (5, 9):                                   # the row's content stream (40) in two slots, whole context
        seed_slot(e, spec, slot, 40, CTX)
    idle = {s: whole_cache(e, spec, s) for s in (0, 3)}
    runs = []
    for slots, rows, x in (([5, 2], [X, A], 0), ([11, 9], [Bc, X], 1), ([2, 5], [A, X], 1)):
        toks, poss = [t for t, _ in rows], [p for _, p in rows]
        lg, _ = e.decode_batch(slots, toks, poss)
        runs.append((lg[x].copy(), whole_cache(e, spec, slots[x])))
        restore(e, spec, slots, poss, streams=[40 if s in (5, 9) else s for s in slots])
    for lg, cache in runs[1:]:
        assert np.array_equal(lg.view(np.uint32), runs[0][0].view(np.uint32))
        assert same_cache(cache, runs[0][1])
    L, nkv, hd, per = geometry(spec)
    assert not np.array_equal(runs[0][1][0][0][X[1]], stream_blocks(40, 0, X[1] + 1, per // 32)[0][X[1]])   # (the row was written)
    for s, before in idle.items():
        assert same_cache(whole_cache(e, spec, s), before), s
    other, _ = e.decode_batch([6, 2], [X[0], A[0]], [X[1], A[1]])     # the same row over ANOTHER slot's content: the cache does reach the logits
    restore(e, spec, [6, 2], [X[1], A[1]])
    print("%s: the row over another cache content: |logits difference| = %.3g" % (name, float(np.abs(other[0] - runs[0][0]).max())))
    assert not np.array_equal(other[0], runs[0][0])
    for slot in (5, 9):
        seed_slot(e, spec, slot, slot, CTX)


# ------------------------------------------------------------------------------------------------ 6. generation
def gen_params(temperature, top_k, top_p, penalty, window=64, seed=42, max_tokens=8, stop_at_eos=False):
    return E.GenParams(max_tokens, temperature, top_k, top_p, penalty, window, seed, int(stop_at_eos))


GREEDY_ROW = gen_params(0.0, 0, 1.0, 1.0, window=0)


def on_device(p, vocab):
    return (p.temperature <= 0.0 or (0 < p.top_k <= 64 and p.top_k < vocab)) and p.repeat_window <= 4096


def python_loop(eng, prompts, params, sampled):
    """generate_batch (sampled=False: decode_batch's greedy tokens) / generate_batch_ex (decode_batch_sample) restated over the public step calls; every
    device-sampled token is checked against nt_sampler_draw_nth on the step's returned logits"""
    n, vocab, ctx = len(prompts), eng.vocab_size, eng.max_context
    seqs, out, taken = [list(p) for p in prompts], [[] for _ in range(n)], [0] * n
    uni = [E.sampler_uniforms(p.seed, p.max_tokens + 1) for p in params]
    pos = [len(p) for p in prompts]

    def host_token(i, logits):
        if not sampled:
            return int(np.argmax(logits))
        tok = E.sampler_draw_nth(logits, params[i], seqs[i], taken[i])
        taken[i] += params[i].temperature > 0.0
        return tok

    for i in range(n):
        tok = host_token(i, eng.seq_forward(i, prompts[i], 0))
        seqs[i].append(tok); out[i].append(tok)
    live = [True] * n
    while True:
        for i in range(n):
            if live[i] and (len(out[i]) >= params[i].max_tokens or pos[i] >= ctx):
                live[i] = False
        rows = [i for i in range(n) if live[i]]
        if not rows:
            return out
        last, poss = [seqs[i][-1] for i in rows], [pos[i] for i in rows]
        if not sampled:
            _, nxt = eng.decode_batch(rows, last, poss, logits=False)
        else:
            row_params, recent, r = [], [], []
            for i in rows:
                p = params[i]
                if on_device(p, vocab):
                    w = max(0, min(len(seqs[i]), p.repeat_window))
                    row_params.append(p); recent.append(seqs[i][len(seqs[i]) - w:]); r.append(uni[i][taken[i]] if p.temperature > 0.0 else 0.0)
                else:
                    row_params.append(GREEDY_ROW); recent.append([]); r.append(0.0)
            lg, dev = eng.decode_batch_sample(rows, last, poss, row_params, recent, r)
            nxt = []
            for b, i in enumerate(rows):
                tok = host_token(i, lg[b])
                if on_device(params[i], vocab):
                    assert dev[b] == tok, (i, len(out[i]))     # the device's token = the host sampler on the step's logits
                nxt.append(tok)
        for b, i in enumerate(rows):
            seqs[i].append(nxt[b]); out[i].append(nxt[b]); pos[i] += 1


def test_generation_runs_through_the_batched_step():
    """generate_batch (greedy) and generate_batch_ex (one greedy row, one sampled with the reference's defaults, one with top_k = 100: the host sampler's
    path) on a q8_0 engine equal the caller-driven loops; the sequence whose prompt ends one row short of the context leaves at the context's end."""
    spec, ctx = tiny128_spec(), 48
    eng = engine(spec, ctx, "q8_0", batch_kv_q8=1, sequences=3)
    r = rng(61)
    prompts = [[int(t) for t in r.integers(0, 500, n)] for n in (5, ctx - 1, 9)]
    greedy = [gen_params(0.0, 40, 0.9, 1.0)] * 3
    got = eng.generate_batch(prompts, 8, stop_at_eos=False)
    assert got == python_loop(eng, prompts, greedy, sampled=False)
    assert [len(s) for s in got] == [8, 2, 8]                     # (prefill's token + the one step at the last position)
    params = [gen_params(0.0, 40, 0.9, 1.0), gen_params(0.7, 40, 0.9, 1.1, seed=1), gen_params(0.9, 100, 0.95, 1.2, seed=2)]
    assert [on_device(p, spec.vocab) for p in params] == [True, True, False]
    got = eng.generate_batch_ex(prompts, params)
    assert got == python_loop(eng, prompts, params, sampled=True)
    assert [len(s) for s in got] == [8, 2, 8] and len(set(got[2])) > 1
    eng.close()


# ------------------------------------------------------------------------------------------------ 7. one row on a one-slot engine
def test_decode_batch_on_a_one_slot_engine():
    spec, ctx = small_spec(), 1024
    prompt = [int(t) for t in rng(71).integers(0, 2000, 600)]
    e = engine(spec, ctx, "q8_0")
    e.forward(prompt, 0)
    with pytest.raises(_lib.NtkError) as ei:
        e.decode_batch([0], [5], [600])
    assert ei.value.status == -2 and "q8_0" in str(ei.value)
    with pytest.raises(_lib.NtkError) as ei:
        e.decode_batch_sample([0], [5], [600], [gen_params(0.7, 40, 0.9, 1.1)], [[1, 2]], [0.5])
    assert ei.value.status == -2
    ref = e.decode_fused(5, 600, False)                           # (the refusals left the engine usable)
    e.close()
    e = engine(spec, ctx, "q8_0", batch_kv_q8=1)
    e.forward(prompt, 0)
    lg, nxt = e.decode_batch([0], [5], [600])
    err = float(np.abs(lg[0] - ref).max())
    print("one slot, position 600: |decode_batch - decode_fused| = %.3g" % err)
    assert err <= 1e-3 and nxt[0] == int(np.argmax(lg[0]))
    p = gen_params(0.7, 40, 0.9, 1.1)
    lg2, tok = e.decode_batch_sample([0], [5], [600], [p], [[1, 2]], [0.5])
    assert np.array_equal(lg2.view(np.uint32), lg.view(np.uint32))
    e.close()
