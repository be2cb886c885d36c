"""The packed prompt pass (nt_engine_forward_batch, option "batch_prefill") on the six golden models, loaded with a context of 256 and six sequence
slots: against one oracle model per prompt, against nt_engine_seq_forward, and against itself under other packings.  TOL and the clear-margin rule are
test_engine_gpu.py's; the cache bars are test_batch_decode_gpu.py's.

Prompts: the golden prompt's first token followed by ids from Philox key [20261019, seed], seeds 21 .. 26, lengths 1, 5, 16, 17, 33, 70.  The oracle
alone, on the CPU, gives every prompt's logits a top-two margin of at least 1.88e-2 on all six models (smallest: small_q4_k_m, seed 21), so no position
falls under the 2 x TOL clear-margin rule: asserted below as "share under the margin == 0"."""
import numpy as np
import pytest

from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from oracle import oracle as O
from test_batch_sampling_gpu import gen_params, python_loop
from test_oracle_golden import CASES, golden_model

pytestmark = pytest.mark.gpu
TOL = 1e-3
CTX = 256
SEEDS = (21, 22, 23, 24, 25, 26)
LENGTHS = (1, 5, 16, 17, 33, 70)
PACKINGS = [(0, 1, 2), (1, 2, 3), (0, 1, 2, 3, 4, 5)]          # 22, 38 and 142 rows: the three GEMM forms (<= 32, 33 .. 64, > 64 rows)

_oracle = {}


def prompts_of(z):
    out = []
    for seed, n in zip(SEEDS, LENGTHS):
        r = np.random.Generator(np.random.Philox(key=[20261019, seed]))
        out.append([int(z["prompt"][0])] + [int(t) for t in r.integers(0, 256, n - 1)])
    return out


def oracle_run(name, path, z):
    """One OracleModel per prompt: its logits and caches; for the 17-token prompt also the decode step behind it (its arg-max at position 17).  Computed
    once per model and shared, read only."""
    if name not in _oracle:
        seqs = []
        for prompt in prompts_of(z):
            m = O.OracleModel(path, CTX)
            lg = m.forward(prompt, 0)
            seq = dict(prompt=prompt, logits=lg, k=[a.copy() for a in m.k_cache], v=[a.copy() for a in m.v_cache])
            if len(prompt) == 17:
                seq["fed"] = m.argmax(lg)
                seq["step"] = m.forward([seq["fed"]], 17)
            seqs.append(seq)
        _oracle[name] = seqs
    return _oracle[name]


_rows = {}


def oracle_row(path):
    """halves per cache row (n_kv_heads * head_dim) of a model"""
    if path not in _rows:
        m = O.OracleModel(path, 4)
        _rows[path] = m.k_cache[0].size // 4
    return _rows[path]


def engine_for(path, sequences=6, ctx=CTX, **opts):
    eng = E.Engine()
    eng.set_option("sequences", sequences)
    for k, v in opts.items():
        eng.set_option(k, v)
    eng.load(path, ctx)
    return eng


def cache_rows(eng, slot, n, row, pos0=0):
    """rows [pos0, pos0 + n) of every layer of a slot: [(k, v)] per layer"""
    return [eng.kv_read_slot(slot, layer, pos0, n, row) for layer in range(eng.n_layers)]


def halves(a):
    return a.view(np.float16).astype(np.float32)


@pytest.mark.parametrize("name,shape,mix", CASES)
def test_three_packings_match_one_oracle_model_per_segment(name, shape, mix, tmp_path):
    """{1, 5, 16}, {5, 16, 17} and all six prompts, one call each, prompt i of the packing in slot i: every segment's logits within TOL of its oracle,
    next = the oracle's arg-max (no position under the margin), the slot caches hold the oracle's rows at 2e-3 max(1, |.|max) for K and V."""
    path, z = golden_model(name, shape, mix, tmp_path)
    seqs = oracle_run(name, path, z)
    margins = [float(np.sort(s["logits"])[-1] - np.sort(s["logits"])[-2]) for s in seqs]
    print(name, "smallest top-two margin:", min(margins))
    assert np.mean([m <= 2 * TOL for m in margins]) == 0          # share under the margin == 0
    eng = engine_for(path)
    row = seqs[0]["k"][0].size // CTX
    for packing in PACKINGS:
        slots = list(range(len(packing)))
        got, nxt = eng.forward_batch(slots, [seqs[i]["prompt"] for i in packing], [0] * len(packing))
        assert sum(LENGTHS[i] for i in packing) in (22, 38, 142) and got.shape == (len(packing), eng.vocab_size) and np.isfinite(got).all()
        for slot, i in enumerate(packing):
            err = float(np.abs(got[slot] - seqs[i]["logits"]).max())
            print(name, packing, "segment", i, "max |dlogit| =", err)
            assert err <= TOL, (name, packing, i, err)
            assert nxt[slot] == int(np.argmax(seqs[i]["logits"])), (name, packing, i)
            n = LENGTHS[i]
            for layer, (k, v) in enumerate(cache_rows(eng, slot, n, row)):
                wk, wv = halves(seqs[i]["k"][layer][: n * row]).reshape(n, row), halves(seqs[i]["v"][layer][: n * row]).reshape(n, row)
                assert np.abs(halves(k) - wk).max() <= 2e-3 * max(1.0, float(np.abs(wk).max())), (packing, i, layer)
                assert np.abs(halves(v) - wv).max() <= 2e-3 * max(1.0, float(np.abs(wv).max())), (packing, i, layer)
    eng.close()


@pytest.mark.parametrize("name,shape,mix", [CASES[0], CASES[3], CASES[4]])
def test_one_segment_leaves_seq_forwards_cache_rows_bit_for_bit(name, shape, mix, tmp_path):
    """forward_batch([s], [p], [0]) on one engine, seq_forward(s, p, 0) on a second: the same cache rows in every layer, bit for bit (the same GEMM form
    for the same row count, the shared rotation and store, the same attention device function); logits within TOL of each other (another LM-head form)."""
    path, z = golden_model(name, shape, mix, tmp_path)
    prompts = prompts_of(z)
    a, b = engine_for(path), engine_for(path)
    row = oracle_row(path)
    # lengths 5, 33 and 70; and 2 and 3, where seq_forward rotates with ntk_rope's per-pair kernel and stores with ntk_copy_to_kv_cache: the same expressions
    for slot, p in ((2, prompts[1]), (0, prompts[4]), (5, prompts[5]), (1, prompts[2][:2]), (3, prompts[2][:3])):
        got, _ = a.forward_batch([slot], [p], [0])
        want = b.seq_forward(slot, p, 0)
        err = float(np.abs(got[0] - want).max())
        print(name, len(p), "max |dlogit| against seq_forward =", err)
        assert err <= TOL, (name, len(p), err)
        for layer, ((ka, va), (kb, vb)) in enumerate(zip(cache_rows(a, slot, len(p), row), cache_rows(b, slot, len(p), row))):
            assert np.array_equal(ka, kb) and np.array_equal(va, vb), (name, len(p), layer)
    a.close(); b.close()


@pytest.mark.parametrize("name,shape,mix", [CASES[1], CASES[3], CASES[5]])
def test_companions_order_offset_and_slot_do_not_matter_and_nothing_else_is_written(name, shape, mix, tmp_path):
    """The 142-row packing in slot and segment order 0 .. 5, and in order (5, 2, 0, 4, 1, 3) with the slots renumbered (the j-th segment in slot j): each
    sequence's logits and cache rows are bit-identical.  A call over slots (0, 2) at starts (3, 40) leaves slots 1 and 3, and the rows of slots 0 and 2
    outside the written ranges, bit-unchanged (all four seeded with kv_write_slot)."""
    path, z = golden_model(name, shape, mix, tmp_path)
    prompts = prompts_of(z)
    row = oracle_row(path)
    a, b = engine_for(path), engine_for(path)
    order = [5, 2, 0, 4, 1, 3]
    la, _ = a.forward_batch(list(range(6)), prompts, [0] * 6)
    lb, _ = b.forward_batch(list(range(6)), [prompts[i] for i in order], [0] * 6)
    for j, i in enumerate(order):
        assert np.array_equal(lb[j].view(np.uint32), la[i].view(np.uint32)), i
        for layer, ((ka, va), (kb, vb)) in enumerate(zip(cache_rows(a, i, LENGTHS[i], row), cache_rows(b, j, LENGTHS[i], row))):
            assert np.array_equal(ka, kb) and np.array_equal(va, vb), (i, layer)
    r = np.random.Generator(np.random.Philox(key=[20261019, 99]))
    seeded = {}
    for slot in range(4):
        for layer in range(a.n_layers):
            k, v = (r.standard_normal((CTX, row)).astype(np.float16).view(np.uint16) for _ in range(2))
            a.kv_write_slot(slot, layer, 0, k, v)
            seeded[(slot, layer)] = (k, v)
    written = {0: (3, LENGTHS[2]), 2: (40, LENGTHS[4])}
    a.forward_batch([0, 2], [prompts[2], prompts[4]], [3, 40])
    for slot in range(4):
        start, n = written.get(slot, (0, 0))
        for layer, (k, v) in enumerate(cache_rows(a, slot, CTX, row)):
            wk, wv = seeded[(slot, layer)]
            keep = np.ones(CTX, bool)
            keep[start:start + n] = False
            assert np.array_equal(k[keep], wk[keep]) and np.array_equal(v[keep], wv[keep]), (slot, layer)
            assert n == 0 or not np.array_equal(k[~keep], wk[~keep])
    a.close(); b.close()


@pytest.mark.parametrize("name,shape,mix", CASES)
def test_a_chunked_prompt_and_a_decode_row_in_one_pass(name, shape, mix, tmp_path):
    """The 70-token prompt into slot 0 as 33 tokens at position 0, then 37 at position 33; in the second call slot 1 -- prefilled with the 17-token prompt
    -- rides along as a one-token segment at position 17, fed the oracle's next token.  Slot 0's logits within TOL of the oracle's 70-token pass, slot
    1's within TOL of the oracle's decode step."""
    path, z = golden_model(name, shape, mix, tmp_path)
    seqs = oracle_run(name, path, z)
    long, mid = seqs[5], seqs[3]
    eng = engine_for(path)
    eng.forward_batch([0, 1], [long["prompt"][:33], mid["prompt"]], [0, 0])
    got, nxt = eng.forward_batch([0, 1], [long["prompt"][33:], [mid["fed"]]], [33, 17])
    e0, e1 = float(np.abs(got[0] - long["logits"]).max()), float(np.abs(got[1] - mid["step"]).max())
    print(name, "chunked prompt max |dlogit| =", e0, " decode row =", e1)
    assert e0 <= TOL and e1 <= TOL, (name, e0, e1)
    assert nxt[0] == int(np.argmax(long["logits"]))
    eng.close()


class PackedPrefill:
    """An engine whose seq_forward(i, prompts[i], 0) answers from ONE forward_batch over all prompts: test_batch_sampling_gpu.python_loop, the restatement of
    generate_batch_ex over the public step calls, then runs with forward_batch in place of its seq_forward loop."""

    def __init__(self, eng, prompts):
        self.eng = eng
        self.rows, _ = eng.forward_batch(list(range(len(prompts))), prompts, [0] * len(prompts))

    def seq_forward(self, slot, tokens, start_pos):
        return self.rows[slot]

    def __getattr__(self, name):
        return getattr(self.eng, name)


@pytest.mark.parametrize("name,shape,mix", [CASES[0], CASES[3]])
def test_the_generators_with_batch_prefill(name, shape, mix, tmp_path):
    """batch_prefill = 1: generate_batch (8 tokens, four prompts) = a Python loop of forward_batch, then decode_batch, taking numpy.argmax, id for id;
    generate_batch_ex at temperature 0.7 = the public-step restatement with forward_batch as its prefill.  Set after the load: read per call."""
    path, z = golden_model(name, shape, mix, tmp_path)
    prompts = prompts_of(z)[1:5]
    n_gen = 8
    eng = engine_for(path, sequences=4)
    lg, nx = eng.forward_batch([0, 1, 2, 3], prompts, [0] * 4)
    last = [int(t) for t in lg.argmax(1)]
    assert last == nx
    streams = [[t] for t in last]
    for i in range(1, n_gen):
        lg, nx = eng.decode_batch([0, 1, 2, 3], last, [len(p) + i - 1 for p in prompts])
        last = [int(t) for t in lg.argmax(1)]
        for s in range(4): streams[s].append(last[s])
    eng.set_option("batch_prefill", 1)
    assert eng.generate_batch(prompts, n_gen, stop_at_eos=False) == streams
    st = eng.stats()
    assert st.prompt_tokens == sum(len(p) for p in prompts) and st.gen_tokens == 4 * (n_gen - 1)
    params = [gen_params(0.7, 40, 0.9, 1.1, seed=s + 1, max_tokens=n_gen) for s in range(4)]
    got = eng.generate_batch_ex(prompts, params)
    want = python_loop(PackedPrefill(eng, prompts), prompts, params, eos=-1)
    assert got == want and all(len(s) == n_gen for s in got)
    with pytest.raises(_lib.NtkError):
        eng.set_option("batch_prefill", 2)
    eng.close()


def test_refusals_leave_the_engine_usable(tmp_path):
    name, shape, mix = CASES[3]                      # small_q8_0: head_dim 128, which the 8-bit cache takes
    path, z = golden_model(name, shape, mix, tmp_path)
    prompts = prompts_of(z)
    # the 8-bit cache, with the slots "batch_kv_q8" gives it
    q8 = engine_for(path, sequences=2, kv_cache="q8_0", batch_kv_q8=1)
    with pytest.raises(_lib.NtkError) as err:
        q8.forward_batch([0, 1], [prompts[1], prompts[2]], [0, 0])
    assert err.value.status == -2 and "q8_0" in str(err.value)
    assert np.isfinite(q8.seq_forward(1, prompts[1], 0)).all()
    q8.set_option("batch_prefill", 1)                # ignored there: the slot-by-slot prefill stays
    assert len(q8.generate_batch([prompts[1], prompts[2]], 3, stop_at_eos=False)[1]) == 3
    q8.close()
    # the ends of the context and of the activation buffers
    ctx = 64
    eng = engine_for(path, sequences=3, ctx=ctx)
    row = oracle_row(path)
    p5, p33 = prompts[1], prompts[4]
    got, _ = eng.forward_batch([1], [p5], [ctx - 5])                       # start + len == max_context
    assert np.isfinite(got).all()
    before = [cache_rows(eng, s, ctx, row) for s in range(3)]
    bad = [([1], [p5], [ctx - 4]),                                         # one more
           ([0, 1], [p33, p33[:32]], [0, 0]),                              # 65 rows in all
           ([0, 1], [p5, p5[:4] + [shape.vocab]], [0, 0]),                 # a token id out of range
           ([0, 1], [p5, [-1]], [0, 0]),
           ([0, 0], [p5, p5], [0, 0]), ([0, 3], [p5, p5], [0, 0]), ([0, 1], [p5, []], [0, 0]), ([0, 1], [p5, p5], [0, -1]), ([], [], [])]
    for slots, lists, starts in bad:
        with pytest.raises(_lib.NtkError) as err:
            eng.forward_batch(slots, lists, starts)
        assert err.value.status == -2, (slots, starts)
    after = [cache_rows(eng, s, ctx, row) for s in range(3)]
    for s in range(3):
        for (k0, v0), (k1, v1) in zip(before[s], after[s]):
            assert np.array_equal(k0, k1) and np.array_equal(v0, v1), s
    got, _ = eng.forward_batch([0, 1], [p33, p33[:31]], [0, 0])            # 64 rows: exactly the context
    assert np.isfinite(got).all()
    eng.close()
