"""nt_sampler_draw_nth (host only): draw number d of the host sampler's stream, taken on its own -- what lets a test (or a caller driving
nt_engine_decode_batch_sample) check one sampled token of a sequence without replaying the whole stream."""
import ctypes as C

import numpy as np
import pytest

from ntransformer_amd import engine as E

N, N_DRAWS = 512, 12
RECENT0 = [7, 300, 7, 41, 511]


def logits_with_dominant_entries():
    r = np.random.Generator(np.random.Philox(key=[20261018, 1]))
    x = (r.standard_normal(N) * 2).astype(np.float32)
    x[[7, 41, 300, 480]] += 7.0          # a few dominant tokens: draws repeat, so the growing window changes the penalised logits
    return x


def stream(logits, p):
    L = E._bind()
    out = (C.c_int * N_DRAWS)()
    rec = (C.c_int * len(RECENT0))(*RECENT0)
    L.nt_sampler_draw.argtypes = [C.c_void_p, C.c_int, C.POINTER(E.GenParams), C.POINTER(C.c_int), C.c_int, C.c_int, C.POINTER(C.c_int)]
    assert L.nt_sampler_draw(logits.ctypes.data_as(C.c_void_p), N, C.byref(p), rec, len(RECENT0), N_DRAWS, out) == N_DRAWS
    return list(out)


@pytest.mark.parametrize("temperature,top_k,top_p,penalty", [(0.7, 40, 0.9, 1.1), (0.0, 40, 0.9, 1.3)])
def test_draw_nth_is_the_nth_draw_of_the_stream(temperature, top_k, top_p, penalty):
    """nt_sampler_draw's n_draws successive tokens (window growing by each) = nt_sampler_draw_nth(skip = d, recent = recent0 + out[:d]) for every d.
    The sampled default settings, and greedy with a penalty -- which takes no draw, so `skip` must not matter."""
    logits = logits_with_dominant_entries()
    p = E.GenParams(0, temperature, top_k, top_p, penalty, 8, 1234, 0)      # repeat_window 8: shorter than the window grows to
    want = stream(logits, p)
    keep = logits.copy()
    for d in range(N_DRAWS):
        assert E.sampler_draw_nth(logits, p, RECENT0 + want[:d], d) == want[d], d
        if temperature <= 0.0:
            assert E.sampler_draw_nth(logits, p, RECENT0 + want[:d], 0) == E.sampler_draw_nth(logits, p, RECENT0 + want[:d], 5) == want[d]
    assert np.array_equal(logits, keep)                                      # the caller's logits are not penalised in place
    if temperature > 0.0:
        assert len(set(want)) > 1 and len(set(want)) < N_DRAWS               # more than one token, and repeats
        # a different position of the stream is a different uniform: some draw changes when `skip` is wrong
        assert any(E.sampler_draw_nth(logits, p, RECENT0 + want[:d], d + 1) != want[d] for d in range(N_DRAWS))


def test_draw_nth_refuses_null_and_negative_arguments():
    L = E._bind()
    logits = logits_with_dominant_entries()
    p = E.GenParams(0, 0.7, 40, 0.9, 1.1, 8, 1, 0)
    out = C.c_int(-7)
    lp = logits.ctypes.data_as(C.c_void_p)
    assert L.nt_sampler_draw_nth(None, N, C.byref(p), None, 0, 0, C.byref(out)) == -5
    assert L.nt_sampler_draw_nth(lp, N, C.byref(p), None, 3, 0, C.byref(out)) == -5
    assert L.nt_sampler_draw_nth(lp, N, C.byref(p), None, 0, -1, C.byref(out)) == -2
    assert out.value == -7
    assert L.nt_sampler_draw_nth(lp, N, C.byref(p), None, 0, 0, C.byref(out)) == 0 and 0 <= out.value < N
