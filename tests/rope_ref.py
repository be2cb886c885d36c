"""A numpy restatement of the rotation with a per-pair frequency table: the reference of the RoPE frequency-scaling tests.

angle of pair i at position pos = (float32)pos * tab[i] * fscale, evaluated left to right in float32 (the kernels' order); cos / sin of that float32
angle are taken in float64 and rounded to float32; the rotation itself runs in float32.  test_rope_scaling_cpu.py makes it a reference: with tab = the
plain frequencies it agrees with oracle.rope to 1e-6.

patch_oracle() gives the engine tests a table-aware oracle without touching oracle/: OracleModel.forward calls the module-level oracle.rope, which the
tests replace by rope_ref bound to the model's table and scale."""
from __future__ import annotations

import functools

import numpy as np


def plain_table(hd: int, theta: float) -> np.ndarray:
    """1 / powf(theta, 2i / hd) in float32: the engine's table for a model without factors.  powf is the correctly rounded one (IEEE libm's, what the
    oracle and the engine's host line call): the power taken in float64 and rounded once.  numpy's own float32 power is a vector routine that is up to
    1 ulp off it -- 4e-4 rad of phase at position 4095 -- so it is not used here."""
    i = np.arange(hd // 2, dtype=np.float32)
    e = (np.float32(2) * i) / np.float32(hd)
    p = np.power(np.float64(np.float32(theta)), e.astype(np.float64)).astype(np.float32)
    return (np.float32(1) / p).astype(np.float32)


def scaled_table(hd: int, theta: float, factors) -> np.ndarray:
    """... divided by the per-pair factors in float32"""
    return (plain_table(hd, theta) / np.asarray(factors, np.float32)).astype(np.float32)


def mixed_factors(hd: int, seed: int) -> np.ndarray:
    """A seeded factor table over ALL pairs: exact 1.0, ramp values in (1, 8) and exact 8.0 in a shuffled order, so the fast pairs are scaled as well"""
    rng = np.random.default_rng(seed)
    n = hd // 2
    f = np.empty(n, np.float32)
    kind = rng.permutation(n) % 3
    f[kind == 0] = 1.0
    f[kind == 1] = rng.uniform(1.05, 7.5, int((kind == 1).sum())).astype(np.float32)
    f[kind == 2] = 8.0
    return f


def rope_ref(q, k, positions, nh, nkv, hd, tab, fscale=1.0, interleaved=False):
    """q [T * nh * hd], k [T * nkv * hd] float32 -> the rotated copies (flat, float32)"""
    pos = np.asarray(positions, np.int64)
    T, half = len(pos), hd // 2
    tab = np.asarray(tab, np.float32)
    assert tab.shape == (half,)
    angle = (pos.astype(np.float32)[:, None] * tab[None, :]).astype(np.float32)
    angle = (angle * np.float32(fscale)).astype(np.float32)                        # [T, half], float32 left to right
    c = np.cos(angle.astype(np.float64)).astype(np.float32)[:, None, :]
    s = np.sin(angle.astype(np.float64)).astype(np.float32)[:, None, :]
    out = []
    for x, n in ((q, nh), (k, nkv)):
        x = np.array(x, np.float32).reshape(T, n, hd)
        if interleaved:
            a, b = x[..., 0::2].copy(), x[..., 1::2].copy()
        else:
            a, b = x[..., :half].copy(), x[..., half:].copy()
        ra = (a * c).astype(np.float32) - (b * s).astype(np.float32)
        rb = (a * s).astype(np.float32) + (b * c).astype(np.float32)
        y = np.empty_like(x)
        if interleaved:
            y[..., 0::2], y[..., 1::2] = ra, rb
        else:
            y[..., :half], y[..., half:] = ra, rb
        out.append(y.reshape(-1))
    return out[0], out[1]


def patch_oracle(monkeypatch, tab, fscale=1.0):
    """oracle.rope (what OracleModel.forward calls: q, k, positions, nh, nkv, hd, theta) -> rope_ref with this table and scale; theta is ignored"""
    from oracle import oracle as O

    def patched(q, k, positions, nh, nkv, hd, theta, fscale_=1.0, interleaved=False):
        return rope_ref(q, k, positions, nh, nkv, hd, tab, fscale, interleaved)

    monkeypatch.setattr(O, "rope", patched)
    return functools.partial(rope_ref, tab=tab, fscale=fscale)
