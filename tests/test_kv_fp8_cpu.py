"""The FP8 (E4M3) KV cache, host side (no GPU needed): the numpy encoder the GPU tests compare against is itself checked against a brute-force
nearest-code search, the decoder round-trips every code, the layout's byte counts, and the option exists."""
import numpy as np
import pytest

from ntransformer_amd import _lib, kv_fp8
from ntransformer_amd import engine as E

CODES = np.arange(256, dtype=np.uint8)
VALUES = kv_fp8.decode_e4m3(CODES).astype(np.float64)
FINITE = CODES[~np.isnan(VALUES)]


def nearest_code(x):
    """brute force over the 254 values: the nearest, of two equally near the one with the even code, beyond +-448 the largest; the sign is x's"""
    if np.isnan(x):
        return 0x7F | (0x80 if np.signbit(x) else 0)
    pos = FINITE[FINITE < 0x80]
    d = np.abs(VALUES[pos] - min(abs(float(x)), 448.0))
    best = pos[d == d.min()]
    code = int(best[best % 2 == 0][0]) if len(best) > 1 else int(best[0])
    return code | (0x80 if np.signbit(x) else 0)


def test_encoder_is_rne_and_saturating_against_a_brute_force_search():
    r = np.random.default_rng(20261126)
    mids = (VALUES[0:0x7E] + VALUES[1:0x7F]) / 2                       # every halfway case between neighbours (exact in float32)
    x = np.concatenate([[0.0, -0.0, 448.0, -448.0, 449.0, -449.0, 464.0, 1e9, -1e9, np.inf, -np.inf, 2.0 ** -9, -2.0 ** -9, 2.0 ** -10, 2.0 ** -11,
                         1e-30, np.nan], mids, -mids, np.nextafter(mids.astype(np.float32), np.float32(np.inf)),
                        r.standard_normal(4000) * r.choice([1e-3, 1.0, 100.0], 4000)]).astype(np.float32)
    got = kv_fp8.encode_e4m3(x)
    want = np.array([nearest_code(v) for v in x], np.uint8)
    assert np.array_equal(got, want), [(float(a), int(b), int(c)) for a, b, c in zip(x, got, want) if b != c][:5]
    assert got[2] == 0x7E and got[4] == 0x7E and got[9] == 0x7E and got[10] == 0xFE and got[1] == 0x80 and got[13] == 0 and got[11] == 1


def test_decode_then_encode_is_the_identity_on_every_finite_code():
    assert len(FINITE) == 254 and VALUES[0x7E] == 448.0 and VALUES[0x01] == 2.0 ** -9 and VALUES[0x08] == 2.0 ** -6
    assert np.array_equal(kv_fp8.encode_e4m3(kv_fp8.decode_e4m3(FINITE)), FINITE)
    assert np.array_equal(kv_fp8.decode_f16(FINITE).view(np.float16).astype(np.float64), VALUES[FINITE])   # every value is a half, exactly
    assert (np.abs(kv_fp8.decode_f16(FINITE).view(np.float16)[FINITE & 0x7F != 0]) >= 2.0 ** -14).all()      # ... and a normal one


@pytest.mark.parametrize("g,want", [((1, 1, 128), 256), ((3, 1, 128), 512), ((4096, 8, 128), 4096 * 1024), ((5, 3, 96), 1536), ((16, 1, 44), 0),
                                    ((0, 1, 128), 0)])
def test_layout_byte_counts(g, want):
    assert kv_fp8.cache_bytes(*g) == want


def test_kv_cache_option_takes_fp8_before_a_load_only():
    eng = E.Engine()
    try:
        eng.set_option("kv_cache", "fp8")
        with pytest.raises(_lib.NtkError) as ei:
            eng.set_option("kv_cache", "bogus")
        assert "bogus" in str(ei.value)
        eng.set_option("kv_cache", "f16")
    finally:
        eng.close()
