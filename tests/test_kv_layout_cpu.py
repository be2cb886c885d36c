"""csrc/kv_layout.h -- the one statement of where KV cache rows lie -- on the CPU (no GPU needed): a stand-alone host program
(tests/kv_layout_check.cpp, nothing but that header) prints its numbers, and they must be the built library's ntk_kv_q8_cache_bytes, the Python
mirror's planes (ntransformer_amd/kv_ops.py) and the totals the engine tests expect of kv_cache_bytes()."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from ntransformer_amd import engine as E
from ntransformer_amd import kv_ops as KO
from ntransformer_amd import kv_q8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (max_seq, n_kv_heads, head_dim): the 256-byte rounding active (1, 3, 17 rows of one head of 128), exact multiples, the engine tests' geometries,
# a head size that is no multiple of 128, a long context; then what the format does not have (0 bytes)
VALID = [(1, 1, 128), (3, 1, 128), (17, 1, 128), (64, 1, 128), (256, 2, 128), (1024, 1, 128), (1024, 2, 128), (4096, 8, 128), (5, 3, 96), (7, 2, 32),
         (131072, 8, 128)]
INVALID = [(16, 1, 48), (0, 1, 128), (16, 0, 128), (-1, 1, 128), (16, 1, 0)]
ROWS = [(0, 1), (0, 0), (1, 2), (2, 1)]   # (pos0, n) asked of every geometry, beside its last row and all of its rows


def compilers():
    env = os.environ.get("CXX")
    return ([env] if env else []) + ["c++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]


@pytest.fixture(scope="module")
def layout(tmp_path_factory):
    """{geometry: (f16 elems, q8 bytes, scale offset)}, {(geometry, pos0, n): the six range numbers}, as the program prints them"""
    exe = str(tmp_path_factory.mktemp("kv_layout") / "kv_layout_check")
    tried = []
    for cxx in compilers():
        if shutil.which(cxx) is None:
            tried.append("%s: not found" % cxx)
            continue
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "kv_layout_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
        if r.returncode == 0:
            break
        tried.append("%s: %s" % (cxx, r.stderr.strip()[-400:]))
    else:
        pytest.fail("no host C++ compiler built tests/kv_layout_check.cpp (the library could not have been built either):\n" + "\n".join(tried))
    args = []
    for g in VALID + INVALID:
        args.append("%d,%d,%d" % g)
        if g in VALID:
            S = g[0]
            args += ["%d+%d" % pn for pn in ROWS + [(S - 1, 1), (0, S)] if pn[0] + pn[1] <= S]
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout
    geoms, rows, g = {}, {}, None
    for line in out.splitlines():
        w = line.split()
        if w[0] == "geom":
            g = tuple(int(x) for x in w[1:4])
            geoms[g] = tuple(int(x) for x in w[4:])
        else:
            rows[(g, int(w[1]), int(w[2]))] = tuple(int(x) for x in w[3:])
    assert set(geoms) == set(VALID + INVALID) and len(rows) >= 4 * len(VALID)
    return geoms, rows


def test_q8_layer_bytes_are_the_librarys(layout):
    geoms, _ = layout
    for g in VALID:
        S, nkv, hd = g
        f16_elems, q8_bytes, scale_off = geoms[g]
        assert q8_bytes == kv_q8.cache_bytes(*g), g
        per = nkv * hd
        assert f16_elems == S * per and scale_off == S * per
        assert q8_bytes % 256 == 0 and 0 <= q8_bytes - S * (per + per // 16) < 256     # both planes fit, less than one rounding unit is padding
    assert any(geoms[g][1] != g[0] * g[1] * g[2] * 17 // 16 for g in VALID), "no geometry with the rounding active"
    for g in INVALID:
        assert geoms[g][1] == 0 and kv_q8.cache_bytes(*g) == 0, g


@pytest.mark.parametrize("g", [(3, 1, 128), (17, 1, 128), (64, 1, 128), (5, 3, 96), (256, 2, 128)])
def test_row_ranges_pick_the_rows_of_the_python_mirrors_planes(layout, g):
    geoms, rows = layout
    S, nkv, hd = g
    per, L = nkv * hd, 2
    layer_bytes, scale_off = geoms[g][1], geoms[g][2]
    r = np.random.Generator(np.random.Philox(key=[20261019, S * per]))
    blocks = r.integers(0, 256, (L, S, per // 32, 34), dtype=np.uint8)           # a random plane image of 2 layers, as canonical blocks ...
    raw = KO.q8_blocks_to_planes(blocks, layer_bytes)                              # ... and as the bytes of the layer buffers
    assert raw.size == L * layer_bytes
    assert np.array_equal(KO.q8_planes_to_blocks(raw, L, S, per), blocks)
    f16 = r.integers(0, 1 << 16, (L, S, per), dtype=np.uint16)
    asked = [(pos0, n) for (gg, pos0, n) in rows if gg == g]
    assert (S - 1, 1) in asked and (0, S) in asked and len(asked) >= 4
    for pos0, n in asked:
        f_off, f_bytes, q_off, q_bytes, s_off, s_bytes = rows[(g, pos0, n)]
        assert s_off == scale_off + pos0 * (per // 32) * 2
        for l in range(L):
            d, q = kv_q8.from_blocks(blocks[l, pos0:pos0 + n])
            layer = raw[l * layer_bytes:(l + 1) * layer_bytes]
            assert layer[q_off:q_off + q_bytes].tobytes() == np.ascontiguousarray(q).tobytes(), (pos0, n, l)
            assert layer[s_off:s_off + s_bytes].tobytes() == np.ascontiguousarray(d).tobytes(), (pos0, n, l)
            assert s_off + s_bytes <= layer_bytes and q_off + q_bytes <= scale_off
            assert f16[l].view(np.uint8).reshape(-1)[f_off:f_off + f_bytes].tobytes() == f16[l, pos0:pos0 + n].tobytes()


def tiny128_spec():   # (tests/test_kv_q8_gpu.py's, restated)
    return E.SynthSpec(256, 512, 2, 2, 1, 512, 4096, 1e-5, 500000.0, 256, 257, b"Q8_0", 20261017)


def test_engine_totals_follow_from_the_layout(layout):
    """kv_cache_bytes() = every slot's K and V (n_layers layer buffers each) + in q8_0 mode ONE one-layer F16 image per side: with the program's numbers
    that is what test_kv_q8_gpu.test_engine_option_accounting_and_debug_access and test_batch_kv_q8_gpu.test_option_accounting_and_debug_access expect"""
    geoms, _ = layout

    def total(spec, ctx, q8, slots):
        hd = spec.hidden // spec.heads
        f16_elems, q8_bytes, _ = geoms[(ctx, spec.kv_heads, hd)]
        return slots * 2 * spec.layers * (q8_bytes if q8 else f16_elems * 2) + (2 * f16_elems * 2 if q8 else 0)

    for spec in (tiny128_spec(), E.synth_spec("small")):                         # test_kv_q8_gpu.py: ctx 1024, one slot, both formats
        L, nkv, hd = spec.layers, spec.kv_heads, spec.hidden // spec.heads
        ctx, per = 1024, nkv * hd
        assert total(spec, ctx, False, 1) == 2 * L * ctx * per * 2
        assert total(spec, ctx, True, 1) == 2 * L * kv_q8.cache_bytes(ctx, nkv, hd) + 2 * ctx * per * 2
    spec, ctx, N = E.synth_spec("small"), 256, 3                                 # test_batch_kv_q8_gpu.py: ctx 256, 3 slots q8_0 / 2 slots f16
    L, nkv, hd = spec.layers, spec.kv_heads, spec.hidden // spec.heads
    per = nkv * hd
    assert total(spec, ctx, True, N) == N * 2 * L * kv_q8.cache_bytes(ctx, nkv, hd) + 2 * ctx * per * 2
    assert total(spec, ctx, False, 2) == 2 * 2 * L * ctx * per * 2
