"""KV cache sequence operations on the CPU (no GPU needed): the host-side argument checks of nt_engine_kv_shift / nt_engine_kv_copy, the generate
loop's discard rule, and the numpy checkers of the context shift (ntransformer_amd/kv_ops.py) against the oracle's own RoPE and against a float64
rotation of the stored 8-bit values."""
import numpy as np
import pytest

from ntransformer_amd import engine as E
from ntransformer_amd import kv_ops as KO
from ntransformer_amd import kv_q8 as Q
from oracle import oracle as O

NTK_E_SHAPE = -2
THETA = 500000.0


# ------------------------------------------------------------------------------------------------ the argument checks
def test_kv_shift_validate_accepts_a_shift_inside_the_context():
    assert E.kv_shift_validate(0, 1, 31, 64, 1, 64) == 0
    assert E.kv_shift_validate(2, 3, 8, 50, 3, 64) == 0
    assert E.kv_shift_validate(0, 0, 64, 64, 1, 64) == 0        # everything dropped: nothing moves, still a valid call


@pytest.mark.parametrize("args,why", [
    ((-1, 1, 8, 50, 3, 64), "slot below 0"),
    ((3, 1, 8, 50, 3, 64), "slot past the last"),
    ((0, -1, 8, 50, 3, 64), "keep < 0"),
    ((0, 1, 0, 50, 3, 64), "discard < 1"),
    ((0, 1, -4, 50, 3, 64), "discard negative"),
    ((0, 30, 21, 50, 3, 64), "keep + discard > n_past"),
    ((0, 1, 8, 65, 3, 64), "n_past beyond the context"),
    ((0, 1, 8, -1, 3, 64), "n_past negative"),
])
def test_kv_shift_validate_refuses(args, why):
    assert E.kv_shift_validate(*args) == NTK_E_SHAPE, why


def test_kv_copy_validate_accepts_rows_inside_the_context():
    assert E.kv_copy_validate(0, 1, 0, 20, 3, 64) == 0
    assert E.kv_copy_validate(2, 0, 44, 20, 3, 64) == 0          # up to the last row


@pytest.mark.parametrize("args,why", [
    ((-1, 1, 0, 20, 3, 64), "source slot below 0"),
    ((3, 1, 0, 20, 3, 64), "source slot past the last"),
    ((0, -1, 0, 20, 3, 64), "destination slot below 0"),
    ((0, 3, 0, 20, 3, 64), "destination slot past the last"),
    ((1, 1, 0, 20, 3, 64), "the same slot"),
    ((0, 1, -1, 20, 3, 64), "pos0 < 0"),
    ((0, 1, 0, -1, 3, 64), "n < 0"),
    ((0, 1, 45, 20, 3, 64), "rows past the context"),
    ((0, 1, 65, 0, 3, 64), "pos0 past the context"),
])
def test_kv_copy_validate_refuses(args, why):
    assert E.kv_copy_validate(*args) == NTK_E_SHAPE, why


def test_context_shift_discard_rule():
    assert E.context_shift_discard(64, 1) == 31
    assert E.context_shift_discard(64, 62) == 1
    assert E.context_shift_discard(3, 1) == 1


# ------------------------------------------------------------------------------------------------ the F16 checker against the oracle's RoPE
@pytest.mark.parametrize("interleaved", [False, True])
@pytest.mark.parametrize("hd", [64, 128])
def test_shift_f16_ref_agrees_with_the_oracle_rope_at_the_new_positions(hd, interleaved):
    """Keys rotated by the oracle's RoPE at positions 8 .. 47, rounded to half and shifted by -8 with the checker, against the oracle's RoPE at positions
    0 .. 39 rounded to half.  Bar per element: 2^-9 max(|a|, |b|) + 2^-24 with (a, b) the pair's unrotated values -- two half roundings of at most
    2^-11 sqrt(2) max each (the stored value, and the checker's result); the F32 angle slack below position 64 is under 64 x 2^-23 rad and does not count."""
    nkv, T = 2, 40
    r = np.random.default_rng(5 + hd + interleaved)
    k = r.standard_normal(T * nkv * hd).astype(np.float32)
    q = np.zeros(T * nkv * hd, np.float32)
    _, k_old = O.rope(q, k, list(range(8, 8 + T)), nkv, nkv, hd, THETA, 1.0, interleaved)
    _, k_new = O.rope(q, k, list(range(0, T)), nkv, nkv, hd, THETA, 1.0, interleaved)
    cache = np.zeros((1, 48, nkv * hd), np.uint16)
    cache[0, 8:48] = k_old.reshape(T, nkv * hd).astype(np.float16).view(np.uint16)
    vc = r.integers(0, 65536, cache.shape).astype(np.uint16)
    got_k, got_v = KO.shift_f16_ref(cache, vc, 8, 0, T, hd, theta=THETA, interleaved=interleaved)
    want = k_new.reshape(T, nkv * hd).astype(np.float16).astype(np.float64)
    got = got_k[0, :T].view(np.float16).astype(np.float64)
    bar = 2.0 ** -9 * KO.pair_max(k.reshape(T, nkv * hd), hd, interleaved) + 2.0 ** -24
    err = np.abs(got - want)
    print("f16 checker vs oracle rope: worst err / bar = %.3f" % float((err / bar).max()))
    assert (err <= bar).all()
    assert np.array_equal(got_k[0, T:], cache[0, T:])                                  # rows outside the destination keep their bits
    assert np.array_equal(got_v[0, :T], vc[0, 8:48]) and np.array_equal(got_v[0, T:], vc[0, T:])


def test_shift_f16_ref_reads_every_source_row_before_it_writes():
    """an overlapping move (40 rows down by 4) equals the same move made from a copy"""
    r = np.random.default_rng(11)
    k = r.standard_normal((2, 64, 128)).astype(np.float16).view(np.uint16)
    v = r.integers(0, 65536, k.shape).astype(np.uint16)
    k1, v1 = KO.shift_f16_ref(k, v, 8, 4, 40, 64, theta=THETA)
    assert np.array_equal(v1[:, 4:44], v[:, 8:48]) and np.array_equal(v1[:, 44:], v[:, 44:]) and np.array_equal(v1[:, :4], v[:, :4])
    assert np.array_equal(k1[:, :4], k[:, :4]) and np.array_equal(k1[:, 44:], k[:, 44:])
    assert not np.array_equal(k1[:, 4:44], k[:, 8:48])                                 # (rotated)


# ------------------------------------------------------------------------------------------------ the Q8 checker
@pytest.mark.parametrize("interleaved", [False, True])
def test_shift_q8_ref_stays_within_a_quantisation_step_of_the_exact_rotation(interleaved):
    """dequantize_exact(shift_q8_ref(blocks)) against the float64 rotation of dequantize_exact(blocks): per element within 0.625 amax / 127, amax the
    rotated block's largest magnitude -- half a quantisation step plus the half-rounded scale's 127 x 2^-11 = 0.062 of a step, with margin.  V blocks
    are unchanged."""
    hd, nkv, S = 128, 2, 48
    r = np.random.default_rng(3 + interleaved)
    d, q = Q.quantize_q8_0(r.standard_normal((2, S, nkv * hd)).astype(np.float32))
    kb = Q.to_blocks(d, q)
    dv, qv = Q.quantize_q8_0(r.standard_normal((2, S, nkv * hd)).astype(np.float32))
    vb = Q.to_blocks(dv, qv)
    src0, dst0, n = 10, 3, 30
    k1, v1 = KO.shift_q8_ref(kb, vb, src0, dst0, n, hd, theta=THETA, interleaved=interleaved)
    exact = KO.rotate_f64(Q.dequantize_exact(kb[:, src0:src0 + n]), dst0 - src0, hd, theta=THETA, interleaved=interleaved)
    got = Q.dequantize_exact(k1[:, dst0:dst0 + n])
    amax = np.abs(exact.reshape(exact.shape[:-1] + (-1, 32))).max(axis=-1)
    bar = np.repeat(0.625 * amax / 127.0, 32, axis=-1)
    err = np.abs(got - exact)
    print("q8 checker vs exact rotation: worst err / bar = %.3f" % float((err / bar).max()))
    assert (err <= bar).all()
    assert np.array_equal(v1[:, dst0:dst0 + n], vb[:, src0:src0 + n])
    keep = np.ones(S, bool)
    keep[dst0:dst0 + n] = False
    assert np.array_equal(k1[:, keep], kb[:, keep]) and np.array_equal(v1[:, keep], vb[:, keep])


def test_pair_freqs_without_a_table_is_the_forward_kernels_expression():
    """1 / (float)pow((double)theta, (double)((2.0f * i) / head_dim)), the expression of the prompt kernels (csrc/attention.hip)"""
    f = KO.pair_freqs(128, THETA)
    for i in (0, 1, 17, 63):
        want = np.float32(1.0) / np.float32(float(np.float32(THETA)) ** float(np.float32(2.0 * i) / np.float32(128)))
        assert f[i] == want
    assert f.dtype == np.float32 and f[0] == 1.0
