"""Scoring without a GPU: the entry points exist, a NULL engine is tolerated, and the float64 reference of the GPU tests (tests/score_ref.py) is right on
rows worked out by hand."""
import ctypes as C
import math

import numpy as np

from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from score_ref import logprob_ref


def test_library_exports_the_scoring_entry_points():
    L = _lib.lib()
    assert hasattr(L, "nt_engine_score_tokens") and hasattr(L, "ntk_logprob_rows")
    assert hasattr(E.Engine, "score") and hasattr(E.Engine, "perplexity")


def test_score_tokens_tolerates_a_null_engine():
    L = E._bind()
    tok, tgt = (C.c_int * 2)(1, 2), (C.c_int * 2)(2, -1)
    lp = (C.c_float * 2)()
    assert L.nt_engine_score_tokens(None, tok, tgt, 2, 0, lp, None) < 0
    assert L.nt_engine_set_option(None, b"score_rows", b"16") < 0


def test_score_rows_option_is_range_checked_before_any_load():
    e = E.Engine()
    e.set_option("score_rows", 1)
    e.set_option("score_rows", 1024)
    for bad in (0, 1025, -3):
        try:
            e.set_option("score_rows", bad)
        except _lib.NtkError as err:
            assert err.status == -2 and "score_rows" in str(err)
        else:
            raise AssertionError("score_rows = %d was accepted" % bad)
    e.close()


def test_logprob_reference_on_hand_computed_rows():
    inf, nan = float("inf"), float("nan")
    rows = np.array([[0.0, 0.0, 0.0, 0.0],             # uniform: -log 4
                     [math.log(1), math.log(2), math.log(3), math.log(2)],   # p = 1/8, 2/8, 3/8, 2/8
                     [5.0, -inf, 5.0, -inf],            # two live entries, tied: first maximum, -log 2
                     [1.0, 2.0, 3.0, 4.0],              # target -1: exactly 0
                     [-inf, -inf, -inf, -inf],          # nothing live: NaN, top-1 0
                     [1.0, nan, 7.0, 0.0],              # a NaN: NaN, and the maximum ignores it
                     [100.0, 20.0, 20.0, 20.0]],        # the others underflow against the peak: log p(peak) = -3 e^-80 ~ 0
                    np.float32)
    targets = [3, 2, 1, 0, 0, 2, 0]
    targets[3] = -1
    lp, top1 = logprob_ref(rows, targets)
    assert abs(lp[0] + math.log(4)) < 1e-15
    assert abs(lp[1] - math.log(3 / 8)) < 1e-7          # (log 2, log 3 were rounded to F32 on the way in)
    assert lp[2] == -inf                                # the target is a dead entry
    assert lp[3] == 0.0
    assert math.isnan(lp[4]) and math.isnan(lp[5])
    assert abs(lp[6] + 3 * math.exp(-80)) < 1e-30      # (-5.4e-35; float64 returns 0)
    assert list(top1) == [0, 2, 0, 3, 0, 2, 0]
    lp2, _ = logprob_ref(rows[2:3], [0])
    assert abs(lp2[0] + math.log(2)) < 1e-15
