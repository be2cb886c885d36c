"""KV cache sequence operations through the engine on the GPU: nt_engine_kv_shift (context shift with K re-rotation) against the model's own RoPE and
against the numpy checkers, the decode step behind a shift, generation past the end of the context ("context_shift"), nt_engine_kv_copy (slot copy),
a shifted slot inside a batched step, a step on one slot of three (its own rows read, no other slot written), the refusals, and the CLI flags.

The model is the tiny head-128 one of tests/test_kv_q8_gpu.py (hidden 256, 2 layers, 2 heads, 1 KV head, vocabulary 512, Q8_0 weights) at a context of 64.

Run on the MI355X box:  python -m pytest tests/test_kv_ops_engine_gpu.py -m gpu -x -q"""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN
from ntransformer_amd import _lib, kv_q8, ops
from ntransformer_amd import engine as E
from ntransformer_amd import kv_ops as KO

pytestmark = pytest.mark.gpu
THETA = 500000.0
CTX, LAYERS, NKV, HD = 64, 2, 1, 128
ROW = NKV * HD


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261019, 1000 + seed]))


def tiny128_spec():
    return E.SynthSpec(256, 512, LAYERS, 2, NKV, 512, 4096, 1e-5, THETA, 256, 257, b"Q8_0", 20261017)


def engine(kv="f16", **opts):
    e = E.Engine()
    e.set_option("synth_threads", 16)
    e.set_option("kv_cache", kv)
    for key, val in opts.items():
        e.set_option(key, val)
    e.load_synthetic(tiny128_spec(), CTX)
    return e


def slots_engine(kv, n):
    return engine(kv, sequences=n, batch_kv_q8=1) if kv == "q8_0" else engine(kv, sequences=n)


def tokens(r, n):
    return [256] + [int(t) for t in r.integers(0, 256, n - 1)]


def engine_table():
    """the engine's frequency table: 1.0f / powf(theta, (2.0f * i) / head_dim) in float32 (csrc/engine/model_load.cpp)"""
    i = np.arange(HD // 2, dtype=np.float32)
    return (np.float32(1.0) / np.power(np.float32(THETA), (np.float32(2.0) * i) / np.float32(HD), dtype=np.float32)).astype(np.float32)


def read_slot(e, kv, slot):
    """the whole cache of one slot: F16 (k, v) uint16 [L, CTX, ROW]; q8_0 (k, v) canonical blocks uint8 [L, CTX, ROW / 32, 34]"""
    ks, vs = [], []
    for l in range(LAYERS):
        k, v = e.kv_read_q8_slot(slot, l, 0, CTX, ROW) if kv == "q8_0" else e.kv_read_slot(slot, l, 0, CTX, ROW)
        ks.append(k)
        vs.append(v)
    return np.stack(ks), np.stack(vs)


def check_k_f16(got, want, unrotated, what):
    """the kernel tests' F16 bar: 2^-10 max(|a|, |b|) + 2^-24 per element, (a, b) the pair's values before the rotation"""
    err = np.abs(got.view(np.float16).astype(np.float64) - want.view(np.float16).astype(np.float64))
    bar = 2.0 ** -10 * KO.pair_max(unrotated.view(np.float16), HD) + 2.0 ** -24
    print("%s: worst err / bar = %.3f" % (what, float((err / bar).max())))
    assert (err <= bar).all()


def check_k_q8(got_blocks, src_blocks, delta, what):
    """the kernel tests' Q8 bar: within 0.625 amax / 127 of the float64 rotation of the dequantised source rows"""
    exact = KO.rotate_f64(kv_q8.dequantize_exact(src_blocks), delta, HD, inv_freq=engine_table())
    amax = np.abs(exact.reshape(exact.shape[:-1] + (-1, 32))).max(axis=-1)
    bar = np.repeat(0.625 * amax / 127.0, 32, axis=-1)
    err = np.abs(kv_q8.dequantize_exact(got_blocks) - exact)
    print("%s: worst err / bar = %.3f" % (what, float((err / bar).max())))
    assert (err <= bar).all()


# ------------------------------------------------------------------------------------------------ against the model's own RoPE
def test_shifted_keys_are_the_keys_the_model_caches_at_the_new_positions():
    """Engine A forwards 40 tokens and shifts them down by 8; engine B forwards tokens 8 .. 39 (and 8 fillers: the same row count, so the same launch
    form; a layer-0 K / V row depends on nothing but its token and position).  Layer 0's K rows 0 .. 31 agree within 2^-9 max(|a|, |b|) + 2^-24 (two half
    roundings), (a, b) B's unrotated k; its V rows are bit-equal.  Pins the direction, the pairing and the engine's frequency table."""
    r = rng(1)
    toks = tokens(r, 40)
    a, b = engine(), engine()
    a.forward(toks, 0)
    assert a.kv_shift(0, 0, 8, 40) == 32
    ka, va = a.kv_read(0, 0, 32, ROW)
    b.kv_inputs_capture(0)
    b.forward(toks[8:] + [int(t) for t in r.integers(0, 256, 8)], 0)
    kb, vb = b.kv_read(0, 0, 32, ROW)
    k_in, _ = b.kv_inputs_read(32, ROW)
    assert np.array_equal(va, vb)
    err = np.abs(ka.view(np.float16).astype(np.float64) - kb.view(np.float16).astype(np.float64))
    bar = 2.0 ** -9 * KO.pair_max(k_in, HD) + 2.0 ** -24
    print("shift vs the model's RoPE: worst err / bar = %.3f" % float((err / bar).max()))
    assert (err <= bar).all()
    assert float(np.abs(ka.view(np.float16).astype(np.float64)).max()) > 0.01      # (not a cache of zeros)
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ against the checkers
@pytest.mark.parametrize("kv", ["f16", "q8_0"])
def test_engine_shift_against_the_checker_and_leaves_everything_else_alone(kv):
    """nt_engine_kv_shift(slot 1, keep 3, discard 8, n_past 50) on a 3-slot engine: the cache read back against the checker applied to the cache read
    back before (the kernel tests' bars); rows below keep, rows from the old n_past - discard upward and the other slots' caches byte-identical."""
    r = rng(2)
    e = slots_engine(kv, 3)
    for s in range(3):
        e.seq_forward(s, tokens(r, 50), 0)
    before = [read_slot(e, kv, s) for s in range(3)]
    assert e.kv_shift(1, 3, 8, 50) == 42
    after = [read_slot(e, kv, s) for s in range(3)]
    for s in (0, 2):
        assert np.array_equal(after[s][0], before[s][0]) and np.array_equal(after[s][1], before[s][1])
    (k0, v0), (k1, v1) = before[1], after[1]
    assert np.array_equal(k1[:, :3], k0[:, :3]) and np.array_equal(k1[:, 42:], k0[:, 42:])
    if kv == "f16":
        want_k, want_v = KO.shift_f16_ref(k0, v0, 11, 3, 39, HD, inv_freq=engine_table())
        assert np.array_equal(v1, want_v)
        check_k_f16(k1[:, 3:42], want_k[:, 3:42], k0[:, 11:50], "engine shift f16")
    else:
        _, want_v = KO.shift_q8_ref(k0, v0, 11, 3, 39, HD, inv_freq=engine_table())
        assert np.array_equal(v1, want_v)
        check_k_q8(k1[:, 3:42], k0[:, 11:50], -8, "engine shift q8_0")
    e.close()


# ------------------------------------------------------------------------------------------------ the step behind a shift
def test_decode_step_behind_a_shift_matches_a_cache_written_from_the_checker():
    """decode_fused at the new position on the shifted engine against a second engine whose cache was written (kv_write) from shift_f16_ref: the
    project's 1e-3 on the logits (the two caches differ by rare neighbouring-half flips)."""
    r = rng(3)
    toks = tokens(r, 50)
    a, b = engine(), engine()
    a.forward(toks, 0)
    k0, v0 = read_slot(a, "f16", 0)
    n_past = a.kv_shift(0, 3, 8, 50)
    assert n_past == 42
    want_k, want_v = KO.shift_f16_ref(k0, v0, 11, 3, 39, HD, inv_freq=engine_table())
    for l in range(LAYERS):
        b.kv_write(l, 0, want_k[l, :n_past], want_v[l, :n_past])
    la = a.decode_fused(77, n_past, graph=True)
    lb = b.decode_fused(77, n_past, graph=True)
    k1, _ = read_slot(a, "f16", 0)
    flips = int((k1[:, :n_past] != want_k[:, :n_past]).sum())
    err = float(np.abs(la - lb).max())
    print("step behind a shift: max |dlogit| = %.3g (bar 1e-3), %d of %d cached K halves differ from the checker's" % (err, flips, k1[:, :n_past].size))
    assert np.isfinite(la).all() and err <= 1e-3
    a.close()
    b.close()


# ------------------------------------------------------------------------------------------------ generation past the context
def caller_driven(e, prompt, n_tokens, keep=1):
    """the generate loop rebuilt from the public calls: prompt pass, first maximum, then decode_greedy_steps up to the end of the context and
    nt_engine_kv_shift with nt_context_shift_discard at every boundary"""
    out = [int(np.argmax(e.forward(prompt, 0)))]
    pos, shifts = len(prompt), 0
    while len(out) < n_tokens:
        if pos >= CTX:
            k = min(keep, CTX - 2)
            pos = e.kv_shift(0, k, E.context_shift_discard(pos, k), pos)
            shifts += 1
        n = min(n_tokens - len(out), CTX - pos)
        out += e.decode_greedy_steps(out[-1], pos, n)
        pos += n
    return out, shifts


@pytest.mark.parametrize("kv,fused", [("f16", 1), ("q8_0", 1), ("f16", 0)])
def test_generation_goes_on_past_the_end_of_the_context(kv, fused):
    """"context_shift" = 1, context 64: generate_tokens (greedy, no EOS stop, 150 tokens behind a 10-token prompt) returns 150 tokens -- with the option
    off it stops at the end of the context, as ever -- and they equal, id for id, the caller-driven loop of decode_greedy_steps + nt_engine_kv_shift at
    the same boundaries (the same kernels on the same inputs)."""
    prompt = tokens(rng(4), 10)
    e = engine(kv, fused=fused, graph=1)
    short = e.generate_tokens(prompt, 150, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False)
    assert len(short) == CTX - len(prompt) + 1                 # today's stop: the context is full
    e.set_option("context_shift", 1)
    got = e.generate_tokens(prompt, 150, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False)
    assert len(got) == 150
    assert got[:len(short)] == short
    want, shifts = caller_driven(e, prompt, 150)
    assert shifts >= 3
    assert got == want
    e.set_option("context_keep", 5)                             # another kept prefix: other boundaries, still the caller-driven loop's tokens
    assert e.generate_tokens(prompt, 150, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False) == caller_driven(e, prompt, 150, keep=5)[0]
    e.set_option("context_shift", 0)
    assert e.generate_tokens(prompt, 150, temperature=0.0, repeat_penalty=1.0, stop_at_eos=False) == short
    e.close()


def test_context_options_are_validated():
    e = E.Engine()
    for key, bad in (("context_shift", "2"), ("context_shift", "yes"), ("context_keep", "-1"), ("context_keep", "x")):
        with pytest.raises(_lib.NtkError) as err:
            e.set_option(key, bad)
        assert err.value.status == -2 and key in str(err.value)
    e.set_option("context_shift", "1")
    e.set_option("context_keep", "0")
    e.close()


# ------------------------------------------------------------------------------------------------ slot copy
@pytest.mark.parametrize("kv", ["f16", "q8_0"])
def test_slot_copy_fills_other_slots_from_a_prefilled_prefix(kv):
    """A 20-token prompt prefilled once into slot 0 and copied to slots 1 and 2: all layers' rows 0 .. 19 byte-equal to slot 0's, the destination
    slots' rows from 20 upward keep what they held, and a decode_batch over the three slots with one token at position 20 gives three bit-identical
    logit rows."""
    r = rng(5)
    e = slots_engine(kv, 3)
    for s in (1, 2):
        e.seq_forward(s, tokens(r, 30), 0)                      # something to keep in rows 20 .. 29
    held = [read_slot(e, kv, s) for s in (1, 2)]
    e.seq_forward(0, tokens(r, 20), 0)
    assert e.kv_copy(0, 1, 0, 20) == 20 and e.kv_copy(0, 2, 0, 20) == 20
    k0, v0 = read_slot(e, kv, 0)
    for (hk, hv), s in zip(held, (1, 2)):
        k, v = read_slot(e, kv, s)
        assert np.array_equal(k[:, :20], k0[:, :20]) and np.array_equal(v[:, :20], v0[:, :20])
        assert np.array_equal(k[:, 20:], hk[:, 20:]) and np.array_equal(v[:, 20:], hv[:, 20:])
        assert not np.array_equal(hk[:, :20], k0[:, :20])
    logits, nxt = e.decode_batch([0, 1, 2], [99, 99, 99], [20, 20, 20])
    assert np.isfinite(logits).all()
    assert np.array_equal(logits[0], logits[1]) and np.array_equal(logits[0], logits[2]) and nxt[0] == nxt[1] == nxt[2]
    e.close()


# ------------------------------------------------------------------------------------------------ a shifted slot in a batch
@pytest.mark.parametrize("kv", ["f16", "q8_0"])
def test_shifting_one_slot_leaves_its_companions_rows_of_a_batched_step_alone(kv):
    """After slot 2 alone was shifted, a decode_batch over slots 0, 1, 2 at their own positions gives slots 0 and 1 the bits of the same step on an
    engine where nothing was shifted."""
    r = rng(6)
    prompts = [tokens(r, 25), tokens(r, 30), tokens(r, 40)]
    x, y = slots_engine(kv, 3), slots_engine(kv, 3)
    for e in (x, y):
        for s, p in enumerate(prompts):
            e.seq_forward(s, p, 0)
    assert x.kv_shift(2, 1, 10, 40) == 30
    lx, _ = x.decode_batch([0, 1, 2], [5, 6, 7], [25, 30, 30])
    ly, _ = y.decode_batch([0, 1, 2], [5, 6, 7], [25, 30, 40])
    assert np.isfinite(lx).all()
    assert np.array_equal(lx[0], ly[0]) and np.array_equal(lx[1], ly[1])
    assert not np.array_equal(lx[2], ly[2])
    x.close()
    y.close()


# ------------------------------------------------------------------------------------------------ a step on one slot of three
@pytest.mark.parametrize("kv", ["f16", "q8_0"])
def test_a_step_on_one_slot_reads_its_own_rows_and_writes_no_other_slot(kv):
    """Three slots hold three different prompts (4, 5, 6 rows, both layers).  A decode_batch on slot 1 alone at position 5 writes row 5 of slot 1 in
    both layers and not one other byte of any slot; its logits are, bit for bit, those of the same step on an engine that holds the same prompt in
    slot 2 behind other neighbours: the step read the rows of the slot it named, in every layer."""
    r = rng(8)
    prompts = [tokens(r, 4), tokens(r, 5), tokens(r, 6)]
    x, y = slots_engine(kv, 3), slots_engine(kv, 3)
    for s, t in ((0, 0), (1, 1), (2, 2)):
        x.seq_forward(s, prompts[t], 0)
    for s, t in ((0, 2), (1, 0), (2, 1)):
        y.seq_forward(s, prompts[t], 0)
    before = [read_slot(x, kv, s) for s in range(3)]
    for a, b in ((0, 1), (0, 2), (1, 2)):
        for l in range(LAYERS):                                   # (row 0 is the shared first token's; rows 1 .. 3 differ slot by slot)
            assert not np.array_equal(before[a][0][l, 1:4], before[b][0][l, 1:4]) and not np.array_equal(before[a][1][l, 1:4], before[b][1][l, 1:4])
    lx, _ = x.decode_batch([1], [77], [5])
    ly, _ = y.decode_batch([2], [77], [5])
    assert np.isfinite(lx).all() and np.array_equal(lx[0].view(np.uint32), ly[0].view(np.uint32))
    after = [read_slot(x, kv, s) for s in range(3)]
    for s in (0, 2):
        assert np.array_equal(after[s][0], before[s][0]) and np.array_equal(after[s][1], before[s][1]), s
    for side in (0, 1):
        rest = [i for i in range(CTX) if i != 5]
        assert np.array_equal(after[1][side][:, rest], before[1][side][:, rest])
        for l in range(LAYERS):
            assert not np.array_equal(after[1][side][l, 5], before[1][side][l, 5]), (side, l)
    x.close()
    y.close()


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_engine_usable():
    r = rng(7)
    e = slots_engine("f16", 3)
    e.seq_forward(1, tokens(r, 50), 0)
    before = read_slot(e, "f16", 1)
    bad_shift = [(-1, 1, 8, 50), (3, 1, 8, 50), (1, -1, 8, 50), (1, 1, 0, 50), (1, 30, 21, 50), (1, 1, 8, 65), (1, 1, 8, -2)]
    for args in bad_shift:
        with pytest.raises(_lib.NtkError) as err:
            e.kv_shift(*args)
        assert err.value.status == -2 and "kv_shift: " in str(err.value), args
    bad_copy = [(-1, 1, 0, 20), (0, 3, 0, 20), (1, 1, 0, 20), (0, 1, -1, 20), (0, 1, 45, 20), (0, 1, 0, -1)]
    for args in bad_copy:
        with pytest.raises(_lib.NtkError) as err:
            e.kv_copy(*args)
        assert err.value.status == -2 and "kv_copy: " in str(err.value), args
    after = read_slot(e, "f16", 1)
    assert np.array_equal(after[0], before[0]) and np.array_equal(after[1], before[1])
    assert e.kv_shift(1, 1, 8, 50) == 42 and e.kv_copy(1, 0, 0, 42) == 42          # the next valid calls work
    assert np.array_equal(read_slot(e, "f16", 0)[0][:, :42], read_slot(e, "f16", 1)[0][:, :42])
    assert np.isfinite(e.decode_batch([0, 1], [5, 6], [42, 42])[0]).all()
    e.close()
    one = engine()                                                # a one-slot engine: slot 0 only
    one.forward(tokens(r, 20), 0)
    assert one.kv_shift(0, 1, 4, 20) == 16
    for call in (lambda: one.kv_shift(1, 1, 4, 20), lambda: one.kv_copy(0, 1, 0, 4)):
        with pytest.raises(_lib.NtkError) as err:
            call()
        assert err.value.status == -2
    one.close()
    tp = E.Engine()
    tp.tp_configure(0, 2)                                         # one rank of two, never connected: refused before any launch
    tp.load(os.path.join(GOLDEN, "tiny_q8_0.gguf"), 64)
    for call, name in ((lambda: tp.kv_shift(0, 1, 4, 20), "kv_shift"), (lambda: tp.kv_copy(0, 0, 0, 4), "kv_copy")):
        with pytest.raises(_lib.NtkError) as err:
            call()
        assert err.value.status == -2 and "tensor parallelism" in str(err.value), name
    tp.close()


# ------------------------------------------------------------------------------------------------ CLI
def test_cli_context_shift_flag():
    """`ntransformer --synthetic tiny:Q8_0 -c 64 -n 150 --context-shift -t 0`: all 150 tokens (the statistics count the 149 behind the first) and no
    `exhausted` line; without the flag the line appears and the run stops at the end of the context."""
    exe = os.path.join(os.path.dirname(E.__file__), "ntransformer")
    assert os.path.exists(exe), "CLI not built"
    base = [exe, "--synthetic", "tiny:Q8_0", "-p", "hi", "-c", "64", "-n", "150", "-t", "0", "--repeat-penalty", "1.0"]
    counts = {}
    for flags in ((), ("--context-shift",), ("--context-shift", "--keep", "4")):
        r = subprocess.run(base + list(flags), capture_output=True, timeout=300)
        txt = (r.stderr + r.stdout).decode("utf-8", "replace")
        assert r.returncode == 0, txt[-2000:]
        m = re.search(r"Decode:\s+(\d+) tokens", txt)
        assert m, txt[-2000:]
        counts[flags] = int(m.group(1))
        assert ("exhausted" in txt) == (not flags), txt[-2000:]
    assert counts[()] < 64
    assert counts[("--context-shift",)] == 149 and counts[("--context-shift", "--keep", "4")] == 149
    r = subprocess.run(base + ["--keep", "-3"], capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "--keep" in r.stderr
