"""Scoring on the GPU: ntk_logprob_rows through the C ABI against a float64 log-softmax of the same F32 logits, and Engine.score against the oracle's
logits at every position (tests/score_ref.py), the KV cache it leaves, chunking, chaining, the 8-bit cache, a shared sequence, refusals and the CLI.

Run on the MI355X box:  python -m pytest tests/test_score_gpu.py -m gpu -x -q"""
import math
import os
import subprocess

import numpy as np
import pytest

from conftest import GOLDEN, ROOT
from ntransformer_amd import _lib, ops
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from ntransformer_amd.ops import DeviceBuffer as DB
from score_ref import MODELS, N_TOKENS, logprob_ref, oracle_all_logits, oracle_case

pytestmark = pytest.mark.gpu
TOL = 1e-3   # the project's logit bar against the oracle (tests/test_engine_gpu.py)


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261018, seed]))


# ------------------------------------------------------------------------------------------------ the kernel
KINDS = ["normal", "peak", "equal", "big", "ninf", "ties", "all_ninf"]


def make_row(r, vocab, kind):
    x = (r.standard_normal(vocab) * 2.0).astype(np.float32)              # N(0, 4)
    if kind == "peak":                                                      # one entry 80 above the rest: every other exponential underflows
        x[r.integers(0, vocab)] = x.max() + 80.0
    elif kind == "equal":
        x[:] = 1.25
    elif kind == "big":                                                     # magnitudes around +-1e4
        x = (np.where(r.random(vocab) < 0.5, -1.0, 1.0) * 1e4 * (1.0 + 0.05 * r.standard_normal(vocab))).astype(np.float32)
    elif kind == "ninf":                                                    # some dead entries (one live one at least)
        dead = r.random(vocab) < 0.3
        dead[r.integers(0, vocab)] = False
        x[dead] = -np.inf
    elif kind == "ties":                                                    # the maximum three times
        x[r.integers(0, vocab, 3)] = np.float32(x.max() + 1.0)
    elif kind == "all_ninf":
        x[:] = -np.inf
    return x


def make_targets(r, n_rows, vocab):
    t = r.integers(0, vocab, n_rows).astype(np.int32)
    t[0::4] = 0
    t[1::4] = vocab - 1
    t[3::4] = -1
    return t


def run_kernel(logits, vocab, ld, targets, with_top1=True, offset=0):
    """logits: float32 [n_rows][ld] host; the device copy starts `offset` floats into its allocation (a row start off the 16-byte grid)"""
    n_rows = logits.shape[0]
    buf = DB(4 * (offset + logits.size) + 64)
    buf.upload(np.ascontiguousarray(logits), 4 * offset)
    lp, t1 = DB.from_numpy(np.full(n_rows, 7.0, np.float32)), DB.from_numpy(np.full(n_rows, -5, np.int32))
    ops.logprob_rows(buf.at(4 * offset), n_rows, vocab, ld, DB.from_numpy(targets), lp, t1 if with_top1 else None)
    return lp.numpy(np.float32, n_rows), t1.numpy(np.int32, n_rows)


def assert_close(got, want):
    """|got - want| <= 1e-5 + 2^-22 |want| on finite rows; NaN where the reference is NaN and nowhere else; infinities equal"""
    got64 = got.astype(np.float64)
    assert np.array_equal(np.isnan(got64), np.isnan(want)), (got64, want)
    fin = np.isfinite(want)
    assert np.array_equal(got64[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    err = np.abs(got64[fin] - want[fin])
    bar = 1e-5 + 2.0 ** -22 * np.abs(want[fin])
    assert (err <= bar).all(), (float(err.max()), float((err / bar).max()))
    return float((err / bar).max()) if fin.any() else 0.0


def ld_of(vocab, kind):
    return {"dense": vocab, "plus3": vocab + 3, "mult4": (vocab + 3) // 4 * 4}[kind]


SHAPES = [(v, k, n) for v in (1, 31, 64, 257, 512, 4099) for k in ("dense", "plus3", "mult4") for n in (1, 3, 65)] + \
         [(128256, k, 3) for k in ("dense", "plus3", "mult4")]


@pytest.mark.parametrize("vocab,ld_kind,n_rows", SHAPES)
def test_logprob_rows_against_float64(vocab, ld_kind, n_rows):
    """Error bar |got - want| <= 1e-5 + 2^-22 |want| on finite rows, from the kernel's arithmetic on the same F32 logits: l - m is one F32 rounding and
    expf is within 2 ulp, so every summand carries <= 3 * 2^-24 relative; all summands are positive, so a fixed-order F32 sum of n <= 2^17 of them adds at
    most (depth of the order) * 2^-24 relative -- 17 + 3 for a tree; this kernel: <= 32 sequential additions of pairwise-summed groups of four per lane (126
    terms at 128 256), 6 butterfly steps and 15 wave merges, each merge two roundings more: < 60 * 2^-24 -- i.e. S is good to about 2^-18 ... 2^-19
    relative = 2 ... 4e-6 absolute in log S, logf adds an ulp of log S (<= 12: 1e-6) and the final subtraction one rounding of the result (the 2^-22 |want|
    term).  A strictly sequential accumulation of 2 000 terms per lane (2 000 * 2^-24 = 1.2e-4 worst case) would NOT fit under this bar; the kernel sums
    pairwise inside a piece and over 1024 lanes so that it does.  Rows cycle through the kinds (N(0, 4), a peak 80 above the rest, all equal, +-1e4, some
    -inf, tied maxima, all -inf -> NaN); targets 0, vocab - 1, random and -1 (exactly 0).  ld > vocab and a start 1 float off the 16-byte grid put row
    starts at every misalignment: the scalar head and tail."""
    r = rng(vocab * 7 + n_rows + len(ld_kind))
    ld = ld_of(vocab, ld_kind)
    logits = np.full((n_rows, ld), np.nan, np.float32)          # the padding must never be read: a NaN there would poison the row
    for i in range(n_rows):
        logits[i, :vocab] = make_row(r, vocab, KINDS[(i + vocab) % len(KINDS)])
    targets = make_targets(r, n_rows, vocab)
    want, want_top1 = logprob_ref(logits[:, :vocab], targets)
    for offset in (0, 1):
        got, top1 = run_kernel(logits, vocab, ld, targets, offset=offset)
        worst = assert_close(got, want)
        print("vocab %d ld %d rows %d offset %d: worst error / bar = %.3f" % (vocab, ld, n_rows, offset, worst))
        assert (got[targets < 0] == 0.0).all() and not np.signbit(got[targets < 0]).any()
        assert np.array_equal(top1, want_top1)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("vocab", [1, 31, 64, 257, 512, 4099, 128256])
def test_logprob_rows_every_kind_at_every_width(kind, vocab):
    r = rng(vocab + 13 * KINDS.index(kind))
    logits = np.stack([make_row(r, vocab, kind) for _ in range(3)])
    targets = np.array([0, vocab - 1, int(r.integers(0, vocab))], np.int32)
    want, want_top1 = logprob_ref(logits, targets)
    got, top1 = run_kernel(logits, vocab, vocab, targets)
    assert_close(got, want)
    assert np.array_equal(top1, want_top1)
    if kind == "all_ninf":
        assert np.isnan(got).all()
    if kind == "ties":
        assert all(top1[i] == np.flatnonzero(logits[i] == logits[i].max())[0] for i in range(3))


@pytest.mark.parametrize("vocab", [257, 128256])
def test_a_nan_logit_poisons_its_own_row_only(vocab):
    r = rng(vocab)
    logits = np.stack([make_row(r, vocab, "normal") for _ in range(5)])
    logits[2, vocab // 3] = np.nan
    targets = r.integers(0, vocab, 5).astype(np.int32)
    want, want_top1 = logprob_ref(logits, targets)
    got, top1 = run_kernel(logits, vocab, vocab, targets)
    assert np.isnan(got[2]) and np.isfinite(np.delete(got, 2)).all()
    assert_close(got, want)
    assert np.array_equal(top1, want_top1)          # (the NaN never wins the maximum)


def test_skipped_rows_and_no_top1():
    """target -1: exactly 0 -- and with no top-1 asked for the row is not read at all (NaN logits there change nothing)"""
    r = rng(5)
    vocab = 4099
    logits = np.stack([make_row(r, vocab, "normal") for _ in range(4)])
    logits[1, :] = np.nan
    targets = np.array([5, -1, -1, vocab - 1], np.int32)
    want, want_top1 = logprob_ref(logits, targets)
    got, top1 = run_kernel(logits, vocab, vocab, targets, with_top1=False)
    assert got[1] == 0.0 and got[2] == 0.0 and (top1 == -5).all()
    assert_close(got, want)
    got, top1 = run_kernel(logits, vocab, vocab, targets)
    assert got[1] == 0.0 and got[2] == 0.0 and np.array_equal(top1, want_top1)


@pytest.mark.parametrize("vocab,n_rows", [(4099, 65), (128256, 3)])
def test_logprob_rows_is_deterministic(vocab, n_rows):
    r = rng(vocab + 1)
    logits = np.stack([make_row(r, vocab, "normal") for _ in range(n_rows)])
    targets = r.integers(0, vocab, n_rows).astype(np.int32)
    a, ta = run_kernel(logits, vocab, vocab, targets)
    b, tb = run_kernel(logits, vocab, vocab, targets)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ta, tb)


def test_logprob_rows_refuses_bad_arguments():
    L = _lib.lib()
    x, t, o = DB(64), DB(64), DB(64)
    assert L.ntk_logprob_rows(None, 1, 4, 4, t.ptr, o.ptr, None, None) == -5
    assert L.ntk_logprob_rows(x.ptr, 1, 4, 4, None, o.ptr, None, None) == -5
    assert L.ntk_logprob_rows(x.ptr, 1, 4, 3, t.ptr, o.ptr, None, None) == -2       # ld < vocab
    assert L.ntk_logprob_rows(x.ptr, 1, 0, 4, t.ptr, o.ptr, None, None) == -2
    assert L.ntk_logprob_rows(x.ptr, -1, 4, 4, t.ptr, o.ptr, None, None) == -2
    assert L.ntk_logprob_rows(x.ptr, 0, 4, 4, t.ptr, o.ptr, None, None) == 0        # nothing to do


# ------------------------------------------------------------------------------------------------ the LM head's GEMM
@pytest.mark.parametrize("mix,rows,width", [("Q8_0", 512, 256), ("Q6_K", 512, 256), ("Q8_0", 2048, 1024), ("Q4_K", 4096, 512), ("Q8_0", 8192, 256)])
def test_gemm_full_form_does_not_depend_on_how_the_tokens_are_cut(mix, rows, width):
    """ntk_gemm_desc.full_form: 200 tokens in one call, and the same tokens in calls of 16, 1, 64, 33, 70 and 16 (every threshold of the forms the launch
    would otherwise choose by token count: 16, 32, 64; 8192 rows: tall enough for the two-chunks-per-workgroup form, here also over a single chunk), give the
    same bits -- and the GEMM's usual accuracy against a float64 product of the dequantised matrix"""
    r = rng(rows + width)
    gt = G.NAME_TO_GGML[mix]
    raw = np.frombuffer(G.synth_tensor(r, gt, rows, width, sigma=0.05), np.uint8)
    deq = G.dequantize(raw, gt, rows * width).reshape(rows, width).astype(np.float64)
    T = 200
    x = r.standard_normal((T, width)).astype(np.float32)
    W, X = DB.from_numpy(raw), DB.from_numpy(x)
    dt = G.GGML_TO_DT[gt]
    whole = DB(T * rows * 4)
    assert ops._gemm_quant_f16([(W, whole, rows, dt)], X, T, width, full_form=True) == 0
    whole = whole.numpy(np.float32, T * rows).reshape(T, rows)
    want = x.astype(np.float64) @ deq.T
    assert np.abs(whole - want).max() <= 4e-6 * math.sqrt(width) * np.abs(want).max()     # the GEMV tolerance of tests/test_gemv_rp.py
    pieces, t0 = DB(T * rows * 4), 0
    for n in (16, 1, 64, 33, 70, 16):
        assert ops._gemm_quant_f16([(W, pieces.at(t0 * rows * 4), rows, dt)], X.at(t0 * width * 4), n, width, full_form=True) == 0
        t0 += n
    assert t0 == T
    pieces = pieces.numpy(np.float32, T * rows).reshape(T, rows)
    assert np.array_equal(whole.view(np.uint32), pieces.view(np.uint32))


# ------------------------------------------------------------------------------------------------ the engine
def load(path, ctx, **options):
    eng = E.Engine()
    for k, v in options.items():
        if k == "kv_cache":
            eng.set_option(k, v)
    eng.load(path, ctx)
    for k, v in options.items():
        if k != "kv_cache":
            eng.set_option(k, v)
    return eng


def check_against_oracle(got, top1, tokens, logits, what):
    """Bar 2 * TOL: the project's logit bar is TOL in the max norm and log-sum-exp is 1-Lipschitz in it, so |d logprob| <= |d l_t| + |d lse| <= 2 TOL"""
    want, want_top1 = logprob_ref(logits, tokens[1:] + [-1])
    assert got.shape == (len(tokens),) and np.isfinite(got).all() and got[-1] == 0.0
    err = float(np.abs(got.astype(np.float64) - want).max())
    top2 = np.sort(logits, axis=1)[:, -2:]
    clear = (top2[:, 1] - top2[:, 0]) > 2 * TOL
    print("%s: max |d logprob| = %.3g, clear-margin rows %d of %d" % (what, err, int(clear.sum()), len(clear)))
    assert err <= 2 * TOL, (what, err)
    assert 2 * int(clear.sum()) >= len(clear), "the prompt's seed leaves too few rows with a clear top-2 margin"
    assert np.array_equal(top1[clear], want_top1[clear])


@pytest.mark.parametrize("name", [m[0] for m in MODELS])
def test_score_matches_the_oracle_at_every_position(name, tmp_path_factory):
    path, ctx, tokens, logits = oracle_case(name, tmp_path_factory)
    eng = load(path, ctx)
    got, top1 = eng.score(tokens, top1=True)
    check_against_oracle(got, top1, tokens, logits, name)
    assert np.array_equal(eng.score(tokens), got)               # without the greedy tokens: the same numbers
    eng.close()


@pytest.mark.parametrize("name", ["tiny_q8_0", "tiny_q4_k_m", "tiny_mixed"])
def test_score_rows_16_and_256_give_identical_bits(name, tmp_path_factory):
    path, ctx, tokens, logits = oracle_case(name, tmp_path_factory)
    eng = load(path, ctx)
    a, ta = eng.score(tokens, top1=True)                         # 256 rows per chunk: one chunk
    eng.set_option("score_rows", 16)                             # 16 + 16 + 8
    b, tb = eng.score(tokens, top1=True)
    eng.set_option("score_rows", 256)
    c, _ = eng.score(tokens, top1=True)
    eng.close()
    print("%s: rows 16 vs 256: max |d| = %.3g" % (name, float(np.abs(a - b).max())))
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(ta, tb)


@pytest.mark.parametrize("how", ["f16_head", "per_token", "f32_mfma"])
def test_the_fallback_heads_meet_the_oracle_bar(how, tmp_path_factory, tmp_path):
    """the LM head where the FP16 GEMM does not take it: a dense F16 head (per-row GEMV), the reference's per-token sequence (batched_prefill = 0) and the
    F32-MFMA form (f16_prefill = 0)"""
    if how == "f16_head":
        path = str(tmp_path / "tiny_f16.gguf")
        G.make_synthetic_llama(path, G.TINY, "F16", seed=20260925)
        ctx, tokens = 128, oracle_case("tiny_q8_0", tmp_path_factory)[2]
        logits = oracle_all_logits(path, ctx, tokens)
        eng = load(path, ctx)
    else:
        path, ctx, tokens, logits = oracle_case("tiny_q8_0", tmp_path_factory)
        eng = load(path, ctx, **({"batched_prefill": 0} if how == "per_token" else {"f16_prefill": 0}))
    eng.set_option("score_rows", 16)
    got, top1 = eng.score(tokens, top1=True)
    check_against_oracle(got, top1, tokens, logits, how)
    eng.close()


@pytest.mark.parametrize("name", ["tiny_q8_0", "small_q4_k_m"])
def test_kv_cache_after_score_is_forwards(name, tmp_path_factory):
    path, ctx, tokens, _ = oracle_case(name, tmp_path_factory)
    shape = next(s for n, s, _ in MODELS if n == name)
    row = shape.kv_heads * (shape.hidden // shape.heads)
    eng = load(path, ctx)
    n = len(tokens)
    eng.score(tokens)
    after_score = eng.decode_fused(7, n)
    kv_score = eng.kv_read(0, 0, n, row)
    eng.score([3] * n)                                           # other rows in the cache in between
    eng.forward(tokens, 0)
    after_forward = eng.decode_fused(7, n)
    kv_forward = eng.kv_read(0, 0, n, row)
    eng.close()
    assert np.array_equal(after_score.view(np.uint32), after_forward.view(np.uint32))
    assert np.array_equal(kv_score[0], kv_forward[0]) and np.array_equal(kv_score[1], kv_forward[1])
    assert kv_score[0].any()


@pytest.mark.parametrize("name", ["tiny_q8_0", "small_q4_k_m"])
def test_chained_scoring_continues_behind_the_first_call(name, tmp_path_factory):
    """the second call attends to the first call's cache rows (another prompt-attention form: bits may differ, the oracle bar holds)"""
    path, ctx, tokens, _ = oracle_case(name, tmp_path_factory)
    eng = load(path, ctx)
    whole = eng.score(tokens)
    eng.score([5] * len(tokens))
    first = eng.score(tokens[:24], 0, targets=tokens[1:25])
    second = eng.score(tokens[24:], 24)
    eng.close()
    err = float(np.abs(np.concatenate([first, second]) - whole).max())
    print("%s chained: max |d| = %.3g" % (name, err))
    assert err <= 2 * TOL and second[-1] == 0.0


def test_score_with_the_8_bit_kv_cache(tmp_path_factory):
    """Recorded, not asserted (DESIGN.md 4.1 records logit spreads of 2e-2 .. 5e-2 of the logits' RMS between the two caches on synthetic weights): the
    distance to the F16-cache scores.  Asserted: finite, and the greedy token on the clear-margin rows."""
    path, ctx, tokens, logits = oracle_case("small_q8_0", tmp_path_factory)
    f16 = load(path, ctx)
    ref = f16.score(tokens)
    f16.close()
    eng = load(path, ctx, kv_cache="q8_0")
    got, top1 = eng.score(tokens, top1=True)
    eng.close()
    _, want_top1 = logprob_ref(logits, tokens[1:] + [-1])
    print("kv_cache=q8_0 vs f16: max |d logprob| = %.3g, mean %.3g; perplexity %.4f vs %.4f"
          % (float(np.abs(got - ref).max()), float(np.abs(got - ref).mean()), math.exp(-got[:-1].mean()), math.exp(-ref[:-1].mean())))
    assert np.isfinite(got).all() and got[-1] == 0.0
    top2 = np.sort(logits, axis=1)[:, -2:]
    # clear against the recorded spread of the two caches, not against TOL: a logit moves by up to 4.5e-2 of the row's RMS (the largest
    # figure of the 8B rows), so a margin beyond twice that cannot flip
    rms = np.sqrt((logits.astype(np.float64) ** 2).mean(axis=1))
    clear = (top2[:, 1] - top2[:, 0]) > 2 * 4.5e-2 * rms
    assert 2 * int(clear.sum()) >= len(clear) and np.array_equal(top1[clear], want_top1[clear])


def test_a_shared_sequence_scores_the_same_bits(tmp_path_factory):
    path, ctx, tokens, _ = oracle_case("tiny_q4_k_m", tmp_path_factory)
    a = load(path, ctx)
    b = E.Engine()
    b.load_shared(a, ctx)
    ga, gb = a.score(tokens), b.score(tokens)
    b.close()
    a.close()
    assert np.array_equal(ga.view(np.uint32), gb.view(np.uint32))


def test_refusals_come_with_a_message(tmp_path_factory):
    path, ctx, tokens, _ = oracle_case("tiny_q8_0", tmp_path_factory)
    eng = load(path, ctx)
    vocab = eng.vocab_size
    for what, call in (("target", lambda: eng.score(tokens, targets=tokens[1:] + [vocab])),
                       ("token", lambda: eng.score([vocab] + tokens[1:])),
                       ("context", lambda: eng.score(tokens, ctx - len(tokens) + 1)),
                       ("context", lambda: eng.score(list(range(ctx + 1))))):
        with pytest.raises(_lib.NtkError) as err:
            call()
        assert err.value.status == -2 and what in str(err.value), str(err.value)
    with pytest.raises(_lib.NtkError) as err:
        eng.score([])
    assert err.value.status == -2 and "no tokens" in str(err.value)
    assert np.isfinite(eng.score(tokens)).all()                  # and the engine goes on working
    eng.close()
    tp = E.Engine()
    tp.tp_configure(0, 2)                                        # one rank of two, never connected: score refuses before any launch
    tp.load(path, ctx)
    with pytest.raises(_lib.NtkError) as err:
        tp.score(tokens)
    assert err.value.status == -2 and "tensor parallelism" in str(err.value)
    tp.close()


def test_perplexity_windows(tmp_path_factory):
    path, ctx, tokens, _ = oracle_case("tiny_q8_0", tmp_path_factory)
    eng = load(path, ctx)
    lp = eng.score(tokens).astype(np.float64)
    ppl, n = eng.perplexity(tokens)
    assert n == len(tokens) - 1 and abs(ppl - math.exp(-lp[:-1].sum() / n)) <= 1e-12 * ppl
    ppl16, n16 = eng.perplexity(tokens, window=16)               # 16 + 16 + 8 tokens, each window from position 0
    parts = [eng.score(tokens[i:i + 16]).astype(np.float64)[:-1].sum() for i in (0, 16, 32)]
    assert n16 == 15 + 15 + 7 and abs(ppl16 - math.exp(-sum(parts) / n16)) <= 1e-12 * ppl16
    eng.close()


def test_cli_perplexity(tmp_path):
    """`ntransformer --perplexity FILE` prints exp(-mean log P) of the file's tokens behind a BOS: the mean over the SCORED positions of
    Engine.score(Engine.tokenize(text)) (the last entry of that array is the unscored 0 of the final token), to 1e-3 relative"""
    exe = os.path.join(ROOT, "ntransformer_amd", "ntransformer")
    model = os.path.join(GOLDEN, "tiny_q8_0.gguf")
    text = ("The quick brown fox jumps over the lazy dog. " * 5)[:200]
    f = tmp_path / "text.txt"
    f.write_text(text)
    r = subprocess.run([exe, "-m", model, "--perplexity", str(f), "-c", "256", "-v"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    line = next(l for l in r.stdout.splitlines() if l.startswith("Perplexity: "))
    ppl, n = float(line.split()[1]), int(line.split()[3])
    assert any(l.startswith("window 0:") for l in r.stdout.splitlines())
    eng = load(model, 256)
    ids = eng.tokenize(text)
    lp = eng.score(ids).astype(np.float64)
    eng.close()
    want = math.exp(-lp[:-1].mean())
    print("CLI perplexity %.4f over %d tokens; Engine.score %.4f over %d" % (ppl, n, want, len(ids) - 1))
    assert n == len(ids) - 1 and abs(ppl - want) <= 1e-3 * want
    eng = load(model, 256)                                      # ... and Engine.perplexity with the CLI's windows: BOS in front of each, every token scored
    for window in (256, 64):
        r = subprocess.run([exe, "-m", model, "--perplexity", str(f), "-c", str(window)], capture_output=True, text=True, timeout=120)
        line = next(l for l in r.stdout.splitlines() if l.startswith("Perplexity: "))
        py, n_py = eng.perplexity(ids[1:], window=window, bos=ids[0])
        assert n_py == int(line.split()[3]) == len(ids) - 1 and abs(float(line.split()[1]) - py) <= 1e-3 * py
    eng.close()
    for bad in (str(tmp_path / "missing.txt"), None):
        if bad is None:
            bad = str(tmp_path / "empty.txt")
            open(bad, "w").close()
        r = subprocess.run([exe, "-m", model, "--perplexity", bad, "-c", "256"], capture_output=True, text=True, timeout=120)
        assert r.returncode == 1 and "Error" in r.stderr
