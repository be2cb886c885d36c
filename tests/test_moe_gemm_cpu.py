"""The grouped expert GEMM without a GPU: ntk_moe_gemm_scratch_bytes and the refusals that return before any launch, the grammar of the engine options
moe_gemm / moe_gemm_min_rows, and csrc/moe_tiles.h -- the cut of the work list into tiles that the kernel's workgroups compute for themselves -- restated
on the host by a stand-alone program (tests/moe_tiles_check.cpp, nothing but that header): over random offset tables with empty experts and counts of
0 / 1 / 16 / 17, every list entry belongs to exactly one tile, no tile spans two experts, and the tile count stays within ceil(T K / 16) + E, the grid."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from ntransformer_amd import _lib, gguf as G, ops
from ntransformer_amd import engine as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NULL, SHAPE, DTYPE, ALIGN = -5, -2, -1, -4


def test_scratch_bytes_and_the_refusals_that_need_no_device():
    L = _lib.lib()
    for T, Ex, K in ((0, 4, 2), (1025, 4, 2), (4, 257, 2), (4, 32, 17), (4, 2, 3), (4, 0, 1)):
        assert ops.moe_gemm_scratch_bytes(T, Ex, K, 768, 2048) == 0
    need = ops.moe_gemm_scratch_bytes(1024, 128, 8, 768, 2048)
    assert 0 <= need <= 1024 * 8 * 768 * 4 * 2          # (0 today; never more than a gate and an up image of act)
    p = 0x10000          # never dereferenced: every call below is refused on its arguments
    q8 = G.DT_Q8_0

    def gate_up(a=p, x=p, g=p, dg=q8, u=p, du=q8, off=p, pr=p, sc=p, sb=1 << 30, T=4, H=64, I=32, Ex=4, K=2):
        return L.ntk_moe_gemm_gate_up(a, x, g, dg, u, du, off, pr, sc, sb, T, H, I, Ex, K, None)

    def down(yy=p, r=p, a=p, d=p, dd=q8, i=p, ww=p, off=p, pr=p, pt=p, T=4, H=64, I=32, Ex=4, K=2):
        return L.ntk_moe_gemm_down(yy, r, a, d, dd, i, ww, off, pr, pt, T, H, I, Ex, K, None)
    for kw in (dict(a=None), dict(x=None), dict(g=None), dict(u=None), dict(off=None), dict(pr=None)):
        assert gate_up(**kw) == NULL, kw
    for kw in (dict(yy=None), dict(r=None), dict(a=None), dict(d=None), dict(i=None), dict(ww=None), dict(off=None), dict(pr=None), dict(pt=None)):
        assert down(**kw) == NULL, kw
    for dt in (G.DT_F16, G.DT_BF16, G.DT_Q4_0, G.DT_Q5_K, G.DT_F32):
        assert gate_up(dg=dt) == DTYPE and gate_up(du=dt) == DTYPE and down(dd=dt) == DTYPE, dt
    for kw in (dict(T=0), dict(T=1025), dict(Ex=257), dict(K=17, Ex=32), dict(K=5), dict(K=0), dict(H=0), dict(I=0)):
        assert gate_up(**kw) == SHAPE and down(**kw) == SHAPE, kw
    assert gate_up(H=48) == SHAPE and gate_up(H=288, dg=G.DT_Q4_K, du=G.DT_Q4_K) == SHAPE and gate_up(H=288, du=G.DT_Q6_K) == SHAPE   # not whole blocks
    assert down(I=40) == SHAPE and down(I=288, dd=G.DT_Q6_K) == SHAPE
    assert gate_up(a=p + 4) == ALIGN and gate_up(x=p + 8) == ALIGN and gate_up(g=p + 1) == ALIGN and gate_up(u=p + 1) == ALIGN
    assert down(a=p + 4) == ALIGN and down(d=p + 1) == ALIGN
    assert gate_up(dg=G.DT_F16, T=0) == DTYPE and gate_up(a=None, dg=G.DT_F16) == NULL          # the GEMV form's order: pointers, types, counts, alignment


def test_option_grammar():
    e = E.Engine()
    for v in ("0", "1", 0, 1):
        e.set_option("moe_gemm", v)
    for v in ("2", "-1", "on", ""):
        with pytest.raises(_lib.NtkError) as ei:
            e.set_option("moe_gemm", v)
        assert ei.value.status == SHAPE and "moe_gemm must be 0 or 1" in str(ei.value)
    for v in ("1", "2", "64", "1024", 16):
        e.set_option("moe_gemm_min_rows", v)
    for v in ("0", "1025", "-3", "8x", "", "many"):
        with pytest.raises(_lib.NtkError) as ei:
            e.set_option("moe_gemm_min_rows", v)
        assert ei.value.status == SHAPE and "moe_gemm_min_rows" in str(ei.value)
    e.set_option("moe_gemm", "1")          # (a refusal leaves the engine usable)
    e.close()


def compilers():
    env = os.environ.get("CXX")
    return ([env] if env else []) + ["c++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]


@pytest.fixture(scope="module")
def tiles_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("moe_tiles") / "moe_tiles_check")
    tried = []
    for cxx in compilers():
        if shutil.which(cxx) is None:
            tried.append("%s: not found" % cxx)
            continue
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "moe_tiles_check.cpp"), "-o", exe], capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        tried.append("%s: %s" % (cxx, r.stderr.strip()[-400:]))
    pytest.fail("no host C++ compiler built tests/moe_tiles_check.cpp (the library could not have been built either):\n" + "\n".join(tried))


def run_tiles(exe, cases):
    """cases: [(E, n_pairs, offsets)] -> [(tile count, bound, [(number, expert, first, end)])]"""
    text = "".join("%d %d %s\n" % (Ex, n, " ".join(str(int(o)) for o in off)) for Ex, n, off in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout
    res = []
    for line in out.splitlines():
        w = line.split()
        if w[0] == "case":
            res.append((int(w[1]), int(w[2]), []))
        else:
            res[-1][2].append(tuple(int(x) for x in w[1:]))
    assert len(res) == len(cases)
    return res


def partitions():
    r = np.random.Generator(np.random.Philox(key=[20261121, 77]))
    cases = []
    for counts in ([0], [1], [16], [17], [0, 16, 0, 1], [17, 0, 0, 33, 16, 1], [16] * 8, [1] * 256, [0] * 255 + [1024 * 16]):
        cases.append(counts)
    for _ in range(60):
        Ex = int(r.integers(1, 257))
        pool = np.asarray([0, 0, 0, 1, 16, 17, 15, 32, 33, int(r.integers(0, 200))])
        counts = r.choice(pool, Ex)
        while counts.sum() > 1024 * 16:
            counts[int(np.argmax(counts))] = 0
        cases.append([int(c) for c in counts])
    return [(len(c), int(np.sum(c)), np.concatenate([[0], np.cumsum(c)])) for c in cases]


def test_every_entry_is_in_exactly_one_tile_of_its_own_expert(tiles_exe):
    cases = partitions()
    for (Ex, n, off), (ntiles, bound, tiles) in zip(cases, run_tiles(tiles_exe, cases)):
        assert bound == (n + 15) // 16 + Ex
        assert ntiles <= bound, (Ex, n, ntiles, bound)
        assert ntiles == sum((int(off[e + 1] - off[e]) + 15) // 16 for e in range(Ex))
        seen = np.zeros(n, np.int32)
        assert [t[0] for t in tiles] == list(range(ntiles))
        for _, e, first, end in tiles:
            assert 0 <= e < Ex and off[e] <= first < end <= off[e + 1] and end - first <= 16, (e, first, end)          # inside ONE expert's range
            assert (first - off[e]) % 16 == 0 and (end - first == 16 or end == off[e + 1])
            seen[first:end] += 1
        assert (seen == 1).all()


def test_a_table_that_is_not_ours_names_entries_of_the_list_or_nothing(tiles_exe):
    n = 40
    cases = [(4, n, [-5, 3, 3, 100, 200]), (3, n, [50, 60, 70, 80]), (3, n, [-100, -50, -1, 0]), (2, n, [30, 10, 20]), (4, n, [0, 40, 0, 40, 0]),
             (2, n, [-2147483648, 2147483647, -2147483648])]
    for (Ex, _, off), (ntiles, bound, tiles) in zip(cases, run_tiles(tiles_exe, cases)):
        for _, e, first, end in tiles:
            assert 0 <= e < Ex and 0 <= first < end <= n and end - first <= 16
            assert max(int(off[e]), 0) <= first and end <= min(int(off[e + 1]), n)
