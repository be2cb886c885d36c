"""nt_batch_validate: the host-side argument checks of nt_engine_decode_batch (Model::validate_batch), which need no device."""
import ctypes as C

import pytest

from ntransformer_amd import engine as E

SHAPE, NULL = -2, -5


def validate(slots, tokens, positions, n=None, sequences=4, max_seq=128, vocab=512):
    L = E._bind()
    ia = lambda xs: None if xs is None else (C.c_int * max(len(xs), 1))(*xs)
    return L.nt_batch_validate(ia(slots), ia(tokens), ia(positions), len(slots) if n is None else n, sequences, max_seq, vocab)


def test_a_valid_batch_passes_in_any_slot_order():
    assert validate([0], [5], [0]) == 0
    assert validate([3, 1, 0, 2], [0, 511, 7, 7], [127, 0, 5, 5]) == 0
    assert validate(list(range(16)), [1] * 16, [2] * 16, sequences=16) == 0


@pytest.mark.parametrize("slots,tokens,positions,kw", [
    ([], [], [], {}),                                        # B = 0
    ([0, 1, 2, 3, 0], [1] * 5, [0] * 5, {}),                 # B > sequences
    (list(range(17)), [1] * 17, [0] * 17, dict(sequences=17)),   # B > 16 whatever the option says
    ([0, 4], [1, 1], [0, 0], {}),                            # a slot >= sequences
    ([-1], [1], [0], {}),
    ([1, 1], [1, 1], [0, 1], {}),                            # the same slot twice
    ([0, 1], [1, 1], [0, 128], {}),                          # a position >= context
    ([0, 1], [1, 1], [-1, 0], {}),
    ([0, 1], [1, 512], [0, 0], {}),                          # a token id out of range
    ([0, 1], [-1, 1], [0, 0], {}),
])
def test_refusals(slots, tokens, positions, kw):
    assert validate(slots, tokens, positions, **kw) == SHAPE


def test_null_arguments():
    assert validate(None, [1], [0], n=1) == NULL
    assert validate([0], None, [0], n=1) == NULL
    assert validate([0], [1], None, n=1) == NULL
