"""ntk_sample_rows_top_k (csrc/sampling_batch.hip) through ops.sample_rows_top_k: every row of a batch, with its own settings, window and draw, gets
the token the host sampler returns on that row's logits (nt_sampler_draw_nth) and the token ntk_sample_top_k returns on a copy of the row; the logits
afterwards are the host-penalised ones bit for bit.  Every comparison is exact."""
import numpy as np
import pytest

from ntransformer_amd import _lib, ops
from ntransformer_amd import engine as E

pytestmark = pytest.mark.gpu
DB = ops.DeviceBuffer

# (temperature, top_k, top_p, repeat_penalty); temperature 0 = greedy
SETTINGS = [(0.0, 40, 0.9, 1.0),        # greedy without a penalty, with an exact tie planted: the lower id must win
            (0.0, 40, 0.9, 1.3),        # greedy with a penalty
            (0.7, 40, 0.9, 1.1), (1.3, 64, 0.5, 1.0), (0.2, 8, 1.0, 1.5), (0.7, 1, 0.9, 1.1), (2.0, 33, 0.95, 1.2)]
PAD = 3
RECENT_LD = 19                          # windows of 0 .. 16 ids at a pitch that is not their length
PAD_BITS = np.array([np.nan, np.inf, np.nan], np.float32).view(np.uint32)


def rng(n_rows, vocab, first):
    return np.random.Generator(np.random.Philox(key=[20261018, (n_rows * 7 + first) * 1000003 + vocab]))


def make_rows(n_rows, vocab, first):
    """Row b: setting (first + b) % 7, a window of (first + 5 b) % 17 ids -- a token named twice, the out-of-range ids -1 and `vocab`, dominant tokens
    among them so that the penalty decides -- and seed 100 + b.  logits [n_rows][vocab + PAD] with NaN / +inf in the pad."""
    r = rng(n_rows, vocab, first)
    logits = np.empty((n_rows, vocab + PAD), np.float32)
    logits[:, :vocab] = (r.standard_normal((n_rows, vocab)) * 3).astype(np.float32)
    logits[:, vocab:].view(np.uint32)[:] = PAD_BITS
    rows = []
    for b in range(n_rows):
        s = (first + b) % len(SETTINGS)
        hot = r.choice(vocab, min(4, vocab), replace=False)
        logits[b, hot] += 6.0
        n_win = (first + 5 * b) % 17
        win = [int(t) for t in r.integers(0, vocab, n_win)]
        for j, t in enumerate(hot[:3]):
            if j < n_win: win[j] = int(t)
        if n_win >= 2: win[-1] = win[0]                       # named twice: penalised twice
        if n_win >= 5: win[3], win[4] = -1, vocab             # skipped
        if s == 0:
            a, c = sorted(int(t) for t in r.choice(vocab, 2, replace=False))
            logits[b, [a, c]] = logits[b, :vocab].max() + 1.0
        rows.append(dict(setting=s, window=win, seed=100 + b))
    return logits, rows


def params_of(row):
    t, k, p, pen = SETTINGS[row["setting"]]
    return E.GenParams(0, t, k, p, pen, 64, row["seed"], 0)


def host_penalised(x, window, penalty):
    """Sampler::apply_repeat_penalty in float32"""
    x = x.copy()
    if penalty > 1.0:
        pen = np.float32(penalty)
        for t in window:
            if 0 <= t < x.size:
                x[t] = x[t] / pen if x[t] > 0 else x[t] * pen
    return x


def launch(logits, rows, windows, draws, vocab):
    """one call: (status, tokens, logits afterwards)"""
    n_rows = len(rows)
    rec = np.full((n_rows, RECENT_LD), 0, np.int32)           # (id 0 beyond a window: reading past n_recent would penalise token 0)
    spec = []
    for b, row in enumerate(rows):
        rec[b, :len(windows[b])] = windows[b]
        t, k, p, pen = SETTINGS[row["setting"]]
        spec.append((t, k, p, pen, float(draws[b]), len(windows[b])))
    d_logits, d_out = DB.from_numpy(logits), DB.from_numpy(np.full(16, -7, np.int32))
    st = ops.sample_rows_top_k(d_logits, n_rows, vocab, logits.shape[1], DB.from_numpy(rec), RECENT_LD, spec, d_out)
    return st, [int(t) for t in d_out.numpy(np.int32)[:n_rows]], d_logits.numpy(np.float32).reshape(logits.shape)


def single_row(x, row, window, draw):
    """ntk_sample_top_k on a copy of the row"""
    t, k, p, pen = SETTINGS[row["setting"]]
    d_out = DB.zeros(64)
    assert ops.sample_top_k(DB.from_numpy(x), x.size, DB.from_numpy(np.asarray(window + [0], np.int32)), len(window), pen, t, k, p, float(draw), d_out) == 0
    return int(d_out.numpy(np.int32)[0])


@pytest.mark.parametrize("vocab", [5, 512, 2049, 128256, 131072])
@pytest.mark.parametrize("n_rows", [1, 2, 16])
def test_every_row_gets_the_host_samplers_token(n_rows, vocab):
    first = {1: 2, 2: 0, 16: 0}[n_rows] + [5, 512, 2049, 128256, 131072].index(vocab) * (n_rows < 16)
    logits, rows = make_rows(n_rows, vocab, first)
    windows = [row["window"] for row in rows]
    draws = [E.sampler_uniforms(row["seed"], 1)[0] for row in rows]
    st, got, after = launch(logits, rows, windows, draws, vocab)
    assert st == 0
    for b, row in enumerate(rows):
        t, k, p, pen = SETTINGS[row["setting"]]
        x = np.ascontiguousarray(logits[b, :vocab])
        assert got[b] == E.sampler_draw_nth(x, params_of(row), windows[b], 0), (b, row)
        want_after = host_penalised(x, windows[b], pen)
        if t > 0.0:
            assert got[b] == single_row(x, row, windows[b], draws[b]), (b, row)
        else:
            assert got[b] == int(np.argmax(want_after)), (b, row)            # the first maximum
        assert np.array_equal(after[b, :vocab].view(np.uint32), want_after.view(np.uint32)), (b, row)
        assert np.array_equal(after[b, vocab:].view(np.uint32), PAD_BITS), b
        if not (pen > 1.0 and len(windows[b]) > 0):
            assert np.array_equal(after[b].view(np.uint32), logits[b].view(np.uint32)), b
    # rows are independent: the same rows in reversed order give the reversed tokens; the same launch twice gives the same tokens
    st, rev, _ = launch(logits[::-1].copy(), rows[::-1], windows[::-1], draws[::-1], vocab)
    assert st == 0 and rev == got[::-1]
    st, again, _ = launch(logits, rows, windows, draws, vocab)
    assert st == 0 and again == got


def test_successive_draws_with_a_growing_window():
    """16 rows at a vocabulary of 512, 8 successive draws per row, each row's window growing by its own tokens (the last 16 kept): draw d = the host
    sampler's draw d.  The rows sampled with (0.7, 40, 0.9, 1.1), (0.2, 8, 1.0, 1.5) and (2.0, 33, 0.95, 1.2) each produce more than one distinct
    token: more than one position of the cumulative walk is taken (at temperature 0.2 it is chiefly the penalty of 1.5 that moves the walk on, token
    after token).  Checked on the CPU with the host sampler alone.  The other sampled rows are not asked to vary: top_k = 1 keeps one candidate (it
    moves only where the penalty dethrones it), and top_p 0.5 over a dominant token may keep one too (row 10 does)."""
    n_rows, vocab, n_draws = 16, 512, 8
    logits, rows = make_rows(n_rows, vocab, 0)
    uni = [E.sampler_uniforms(row["seed"], n_draws) for row in rows]
    windows = [list(row["window"]) for row in rows]
    streams = [[] for _ in rows]
    for d in range(n_draws):
        wins = [w[-16:] for w in windows]
        st, got, _ = launch(logits, rows, wins, [u[d] for u in uni], vocab)   # (fresh logits per draw: the penalty is applied in place)
        assert st == 0
        for b, row in enumerate(rows):
            assert got[b] == E.sampler_draw_nth(logits[b, :vocab], params_of(row), wins[b], d), (b, d, row)
            windows[b].append(got[b]); streams[b].append(got[b])
    varied = [b for b, row in enumerate(rows) if row["setting"] in (2, 4, 6)]
    assert len(varied) == 6 and all(len(set(streams[b])) > 1 for b in varied), streams


def test_greedy_rows_treat_nan_as_the_host_argmax_does():
    """Sampler::argmax starts at id 0 and moves on l[i] > l[best]: a NaN above id 0 never wins, a NaN AT id 0 is never left.  Rows: NaN at id 0; NaN
    at id 0 under a penalty that names it; NaN at the maximum's id (the runner-up wins); NaN at id 0 of the second chunk and the last id; no NaN."""
    vocab, n_rows = 2049, 5
    r = rng(n_rows, vocab, 99)
    logits = np.zeros((n_rows, vocab + PAD), np.float32)
    logits[:, :vocab] = (r.standard_normal((n_rows, vocab)) * 3).astype(np.float32)
    logits[:, vocab:].view(np.uint32)[:] = PAD_BITS
    logits[0, 0] = logits[1, 0] = np.nan
    logits[2, int(np.argmax(logits[2, :vocab]))] = np.nan
    logits[3, [2048, 700]] = np.nan
    rows = [dict(setting=s, window=w, seed=1) for s, w in ((0, []), (1, [0, 5, 0]), (0, []), (1, [700, 3]), (0, []))]
    windows = [row["window"] for row in rows]
    st, got, after = launch(logits, rows, windows, [0.0] * n_rows, vocab)
    assert st == 0
    for b, row in enumerate(rows):
        x = np.ascontiguousarray(logits[b, :vocab])
        assert got[b] == E.sampler_draw_nth(x, params_of(row), windows[b], 0), (b, got)
        want_after = host_penalised(x, windows[b], SETTINGS[row["setting"]][3])
        np.testing.assert_array_equal(after[b, :vocab], want_after)            # (a NaN stays one; its payload is not pinned)
    assert got[0] == 0 and got[1] == 0 and got[4] == int(np.argmax(logits[4, :vocab]))
    assert got[2] == int(np.nanargmax(logits[2, :vocab]))


def test_refusals_launch_nothing():
    vocab, n_rows = 512, 2
    logits, _ = make_rows(n_rows, vocab, 1)
    d_logits, d_out = DB.from_numpy(logits), DB.from_numpy(np.full(16, -7, np.int32))
    rec = DB.from_numpy(np.zeros((n_rows, RECENT_LD), np.int32))
    ld = vocab + PAD

    def spec(top_k=40, n_recent=6, temperature=0.7):
        return [(0.0, 0, 0.9, 1.3, 0.0, 1), (temperature, top_k, 0.9, 1.1, 0.5, n_recent)]

    def call(n=n_rows, v=vocab, pitch=ld, recent=rec, recent_ld=RECENT_LD, rows_=None, **kw):
        return ops.sample_rows_top_k(d_logits, n, v, pitch, recent, recent_ld, rows_ or spec(), d_out, **kw)

    for name in ("logits", "rows", "d_out", "scratch"):
        assert call(null=(name,)) == -5, name
    assert call(recent=None) == -5                            # a penalty with no windows
    for bad in (dict(n=0), dict(n=17), dict(pitch=vocab - 1), dict(v=131073, pitch=131073), dict(rows_=spec(top_k=0)), dict(rows_=spec(top_k=65)),
                dict(rows_=spec(n_recent=-1)), dict(rows_=spec(n_recent=RECENT_LD + 1))):
        assert call(**bad) == -2, bad
    assert np.all(d_out.numpy(np.int32) == -7)                # nothing ran
    assert np.array_equal(d_logits.numpy(np.float32).view(np.uint32), logits.reshape(-1).view(np.uint32))
    assert call(rows_=spec(top_k=0, temperature=0.0)) == 0    # a greedy row's top_k is not looked at
    assert np.all(d_out.numpy(np.int32)[:n_rows] >= 0)
