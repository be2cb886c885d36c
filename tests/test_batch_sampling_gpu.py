"""Sampled batched decoding (nt_engine_decode_batch_sample / nt_engine_generate_batch_ex) on the golden models: the sampled stream = the host sampler
on the batched step's logits.  Every comparison is exact -- tokens against nt_sampler_draw_nth on the logits the step itself returned, logits against
nt_engine_decode_batch's bits."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

from ntransformer_amd import _lib, gguf as G
from ntransformer_amd import engine as E
from test_oracle_golden import CASES, golden_model

pytestmark = pytest.mark.gpu
TINY, SMALL = CASES[1], CASES[3]          # tiny_q4_k_m (vocab 512), small_q8_0 (vocab 2048)
SEEDS = (11, 12, 13)                      # test_batch_decode_gpu.prompts_of, re-stated: the golden prompt and three seeded ones of lengths 5, 9, 14
LENGTHS = (5, 9, 14)
N_GEN = 10


def prompts_of(z):
    out = [[int(t) for t in z["prompt"]]]
    for seed, n in zip(SEEDS, LENGTHS):
        r = np.random.Generator(np.random.Philox(key=[20261018, seed]))
        out.append([int(z["prompt"][0])] + [int(t) for t in r.integers(0, 256, n - 1)])
    return out


def engine_for(path, z, sequences=4):
    eng = E.Engine()
    eng.set_option("sequences", sequences)
    eng.load(path, int(z["ctx"]))
    return eng


def gen_params(temperature, top_k, top_p, penalty, window=64, seed=42, max_tokens=N_GEN, stop_at_eos=False):
    return E.GenParams(max_tokens, temperature, top_k, top_p, penalty, window, seed, int(stop_at_eos))


GREEDY_ROW = gen_params(0.0, 0, 1.0, 1.0, window=0)      # how a row sampled on the host goes to the device


def on_device(p, vocab):
    """Model::device_sampler_supports and the window cap"""
    return (p.temperature <= 0.0 or (0 < p.top_k <= 64 and p.top_k < vocab)) and p.repeat_window <= 4096


def python_loop(eng, prompts, params, eos):
    """generate_batch_ex restated over the public step calls: seq_forward + the host sampler for each first token, then decode_batch_sample over the live
    slots with the k-th uniform of each sequence's own stream; a sequence the device sampler does not take goes as a greedy row and is sampled by
    nt_sampler_draw_nth from the returned logits.  Every device token is also checked against the host sampler on the step's logits."""
    n, vocab, ctx = len(prompts), eng.vocab_size, eng.max_context
    seqs = [list(p) for p in prompts]
    out = [[] for _ in range(n)]
    taken = [0] * n                                       # uniforms consumed per sequence: one per SAMPLED token
    uni = [E.sampler_uniforms(p.seed, p.max_tokens + 1) for p in params]
    pos = [len(p) for p in prompts]

    def host_token(i, logits):
        tok = E.sampler_draw_nth(logits, params[i], seqs[i], taken[i])
        taken[i] += params[i].temperature > 0.0
        return tok

    for i in range(n):
        tok = host_token(i, eng.seq_forward(i, prompts[i], 0))
        seqs[i].append(tok); out[i].append(tok)
    live = [True] * n
    while True:
        for i in range(n):
            if live[i] and ((params[i].stop_at_eos and out[i][-1] == eos) or len(out[i]) >= params[i].max_tokens or pos[i] >= ctx):
                live[i] = False
        rows = [i for i in range(n) if live[i]]
        if not rows:
            return out
        row_params, recent, r = [], [], []
        for i in rows:
            p = params[i]
            if on_device(p, vocab):
                w = max(0, min(len(seqs[i]), p.repeat_window))
                row_params.append(p); recent.append(seqs[i][len(seqs[i]) - w:]); r.append(uni[i][taken[i]] if p.temperature > 0.0 else 0.0)
            else:
                row_params.append(GREEDY_ROW); recent.append([]); r.append(0.0)
        lg, nxt = eng.decode_batch_sample(rows, [seqs[i][-1] for i in rows], [pos[i] for i in rows], row_params, recent, r)
        for b, i in enumerate(rows):
            tok = host_token(i, lg[b])
            if on_device(params[i], vocab):
                assert nxt[b] == tok, (i, len(out[i]))
            seqs[i].append(tok); out[i].append(tok); pos[i] += 1


MIXED = [[gen_params(0.0, 40, 0.9, 1.3), gen_params(0.7, 40, 0.9, 1.1, seed=1), gen_params(1.3, 64, 0.5, 1.0, seed=2), gen_params(0.2, 8, 1.0, 1.5, seed=3)],
         [gen_params(2.0, 33, 0.95, 1.2, seed=4), gen_params(0.0, 40, 0.9, 1.0), gen_params(0.7, 1, 0.9, 1.1, seed=5), gen_params(0.7, 40, 0.9, 1.1, seed=6)]]


@pytest.mark.parametrize("name,shape,mix", [TINY, SMALL])
def test_a_sampled_step_is_the_host_sampler_on_decode_batchs_logits(name, shape, mix, tmp_path):
    """Four prefilled sequences, one step with mixed per-row settings (twice, at successive positions, to cover all seven): logits_out = decode_batch's
    logits for the same arguments bit for bit (the copy is queued ahead of the in-place penalty), every row's token = nt_sampler_draw_nth on its
    logits_out row with the window and draw the row was given, and a following decode_batch of the same step returns the same logits again."""
    path, z = golden_model(name, shape, mix, tmp_path)
    prompts = prompts_of(z)
    eng = engine_for(path, z)
    for s, p in enumerate(prompts):
        eng.seq_forward(s, p, 0)
    order = [2, 0, 3, 1]
    fed = {s: [int(p[1]), int(p[2])] for s, p in enumerate(prompts)}
    for step, params in enumerate(MIXED):
        toks = [fed[s][step] for s in order]
        poss = [len(prompts[s]) + step for s in order]
        recent = [(prompts[s] + fed[s][:step + 1])[-(3 + 4 * j):] for j, s in enumerate(order)]      # windows of 3, 7, 11 and 15 ids, repeats among them
        skip = 2 + step
        r = [E.sampler_uniforms(p.seed, skip + 1)[skip] for p in params]
        ref, greedy = eng.decode_batch(order, toks, poss)
        lg, nxt = eng.decode_batch_sample(order, toks, poss, params, recent, r)
        assert np.array_equal(lg.view(np.uint32), ref.view(np.uint32))
        for j, p in enumerate(params):
            assert nxt[j] == E.sampler_draw_nth(lg[j], p, recent[j], skip), (step, j)
        if step == 1:
            assert nxt[1] == greedy[1]                                                         # the greedy row without a penalty: decode_batch's first maximum
        none, nxt2 = eng.decode_batch_sample(order, toks, poss, params, recent, r, logits=False)
        assert none is None and nxt2 == nxt
        again, _ = eng.decode_batch(order, toks, poss)
        assert np.array_equal(again.view(np.uint32), ref.view(np.uint32))
    eng.close()


@pytest.mark.parametrize("name,shape,mix", [TINY, SMALL])
def test_generate_batch_ex_equals_the_python_loop(name, shape, mix, tmp_path):
    """Per-sequence seeds and settings, 10 tokens each: the default sampling, top_k = 100 (beyond the device sampler: that sequence's host sampler takes
    its row), greedy with a penalty, and a hot sequence with a 4-token window.  Token for token the Python loop's streams."""
    path, z = golden_model(name, shape, mix, tmp_path)
    prompts = prompts_of(z)
    params = [gen_params(0.7, 40, 0.9, 1.1, seed=1), gen_params(0.9, 100, 0.95, 1.2, seed=2), gen_params(0.0, 40, 0.9, 1.3),
              gen_params(1.5, 40, 1.0, 1.1, window=4, seed=7)]
    assert [on_device(p, shape.vocab) for p in params] == [True, False, True, True]
    eng = engine_for(path, z)
    got = eng.generate_batch_ex(prompts, params)
    st = eng.stats()
    assert st.prompt_tokens == sum(len(p) for p in prompts) and st.gen_tokens == 4 * (N_GEN - 1) and st.decode_tok_s > 0
    want = python_loop(eng, prompts, params, eos=-1)
    assert got == want and all(len(s) == N_GEN for s in got)
    assert len(set(got[0])) > 1 and len(set(got[3])) > 1
    eng.close()


def test_equal_seeds_give_equal_streams_and_different_seeds_differ(tmp_path):
    """Two slots with the same prompt, settings and seed produce identical streams; the same pair with different seeds differs somewhere.  Temperature 1.5
    with top_k 40: 10 draws from a flat distribution over 40 candidates -- that two seeds agree on all ten was ruled out on the CPU with the host sampler
    on the oracle's logits when this test was written (those streams differ from the first token on)."""
    name, shape, mix = TINY
    path, z = golden_model(name, shape, mix, tmp_path)
    prompt = prompts_of(z)[2]
    eng = engine_for(path, z)
    a, b = eng.generate_batch_ex([prompt, prompt], [gen_params(1.5, 40, 1.0, 1.1, seed=5)] * 2)
    assert a == b and len(a) == N_GEN
    c, d = eng.generate_batch_ex([prompt, prompt], [gen_params(1.5, 40, 1.0, 1.1, seed=5), gen_params(1.5, 40, 1.0, 1.1, seed=6)])
    assert c == a and d != c
    eng.close()


def test_sequences_leave_at_their_own_max_tokens_and_eos(tmp_path):
    """max_tokens (3, 10, 6, 10) and the EOS id set to the token sequence 1 produces fourth: every sequence leaves on its own -- at its budget or at EOS
    (written) -- and the others continue unchanged; out_counts (the lengths returned) and the summed stats are right; the Python loop, leaving the same
    way, gives the same streams."""
    name, shape, mix = TINY
    path, z = golden_model(name, shape, mix, tmp_path)
    prompts = prompts_of(z)
    budget = (3, 10, 6, 10)
    settings = [(0.7, 40, 0.9, 1.1), (1.3, 64, 0.95, 1.0), (0.0, 40, 0.9, 1.3), (0.7, 40, 0.9, 1.1)]
    make = lambda stop, budgets: [gen_params(*s, seed=20 + i, max_tokens=budgets[i], stop_at_eos=stop) for i, s in enumerate(settings)]
    eng = engine_for(path, z)
    full = eng.generate_batch_ex(prompts, make(False, (N_GEN,) * 4))
    eng.close()
    eos = full[1][3]
    cut = [s[:m] for s, m in zip(full, budget)]
    cut = [s[: s.index(eos) + 1] if eos in s else s for s in cut]
    assert len(cut[0]) <= 3 and len(cut[1]) <= 4 and max(len(c) for c in cut) > len(cut[1])
    path2 = str(tmp_path / "eos.gguf")
    G.make_synthetic_llama(path2, dataclasses.replace(shape, eos=eos), mix, seed=20260925)
    eng = engine_for(path2, z)
    got = eng.generate_batch_ex(prompts, make(True, budget))
    assert eng.stats().gen_tokens == sum(len(c) - 1 for c in got)
    assert got == python_loop(eng, prompts, make(True, budget), eos)
    assert got == cut
    eng.close()


def test_all_greedy_rows_equal_generate_batch(tmp_path):
    name, shape, mix = TINY
    path, z = golden_model(name, shape, mix, tmp_path)
    prompts = prompts_of(z)
    eng = engine_for(path, z)
    want = eng.generate_batch(prompts, N_GEN, stop_at_eos=False)
    assert eng.generate_batch_ex(prompts, [gen_params(0.0, 40, 0.9, 1.0, seed=i) for i in range(4)]) == want
    eng.close()


def test_refusals_leave_the_engine_usable(tmp_path):
    name, shape, mix = TINY
    path, z = golden_model(name, shape, mix, tmp_path)
    prompts = prompts_of(z)[:2]
    eng = engine_for(path, z, sequences=2)
    for s, p in enumerate(prompts):
        eng.seq_forward(s, p, 0)
    args = ([0, 1], [3, 4], [len(p) for p in prompts])
    ref, _ = eng.decode_batch(*args)
    ok = gen_params(0.7, 40, 0.9, 1.1)
    for params, recent in (([ok, gen_params(0.7, 0, 0.9, 1.1)], [[1, 2], [3]]), ([ok, gen_params(0.7, 65, 0.9, 1.1)], [[1, 2], [3]]),
                           ([ok, ok], [[1, 2], [7] * 5000])):
        with pytest.raises(_lib.NtkError) as err:
            eng.decode_batch_sample(*args, params, recent, [0.5, 0.5])
        assert err.value.status == -2
    with pytest.raises(_lib.NtkError) as err:
        eng.generate_batch_ex(prompts + [prompts[0]], [ok] * 3)                               # n above `sequences`
    assert err.value.status == -2
    # an out_stride below one sequence's max_tokens (the Python wrapper sizes it itself: the C call)
    rows = [(C.c_int * len(q))(*q) for q in prompts]
    ptrs = (C.POINTER(C.c_int) * 2)(*[C.cast(r, C.POINTER(C.c_int)) for r in rows])
    lens = (C.c_int * 2)(*[len(q) for q in prompts])
    pa = (E.GenParams * 2)(gen_params(0.7, 40, 0.9, 1.1, max_tokens=4), gen_params(0.7, 40, 0.9, 1.1, max_tokens=9))
    out, counts = (C.c_int * 16)(*([-7] * 16)), (C.c_int * 2)()
    assert eng.L.nt_engine_generate_batch_ex(eng.h, ptrs, lens, 2, pa, out, 8, counts) == -2
    assert list(out) == [-7] * 16
    for s, p in enumerate(prompts):                                                            # still usable: the same bits
        eng.seq_forward(s, p, 0)
    again, _ = eng.decode_batch(*args)
    assert np.array_equal(again.view(np.uint32), ref.view(np.uint32))
    lg, nxt = eng.decode_batch_sample(*args, [ok, ok], [[1, 2], [3]], [0.5, 0.5])
    assert np.array_equal(lg.view(np.uint32), ref.view(np.uint32)) and all(0 <= t < shape.vocab for t in nxt)
    eng.close()
