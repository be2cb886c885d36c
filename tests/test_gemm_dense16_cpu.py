"""The 16-bit matrix-core prompt GEMM (csrc/gemm_dense16.hip) on the CPU -- no GPU needed:

  * the three-piece bfloat16 split of an activation (tests/bf16_split_ref.py, the numpy restatement of the kernel's pre-pass): every piece is a bfloat16 and
    the pieces add up to x exactly wherever x's last bit is at least the smallest bfloat16 subnormal;
  * the launch plan (csrc/gemm_dense16_plan.h) through a stand-alone host program (tests/gemm_dense16_plan_check.cpp, nothing but that header), which walks
    every workgroup of the planned grid the way the kernel numbers it: the tiles cover every (row, token) exactly once, LDS stays within the CU's 160 KiB,
    the workspace is at least what the launch addresses, and every refusal of include/ntk_engine.h is returned."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import bf16_split_ref as S
from ntransformer_amd import gguf as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, BF16 = int(G.DT_F16), int(G.DT_BF16)
E_DTYPE, E_SHAPE, E_ALIGN = -1, -2, -4


# ------------------------------------------------------------------------------------------------ the split
def split_inputs():
    r = np.random.Generator(np.random.Philox(key=[20261021, 1]))
    n = 100000
    bits = (r.integers(0, 2, n, dtype=np.uint32) << np.uint32(31)) | (r.integers(0, 255, n, dtype=np.uint32) << np.uint32(23)) | r.integers(0, 1 << 23, n, dtype=np.uint32)
    edge = np.array([0x7F7FFFFF, 0xFF7FFFFF, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x007FFFFF, 0x00400000, 0x0000FFFF, 0x00010000, 0x00008000,
                     0x00018000, 0x3FFFFFFF, 0xBFFFFFFF, 0x7F7F8000, 0x7F7F7FFF, 0x00FFFFFF, 0x0C7FFFFF, 0x3F800001, 0x3F808000, 0x3F818000], np.uint32)
    full = (r.integers(1, 255, 2000, dtype=np.uint32) << np.uint32(23)) | np.uint32(0x7FFFFF)      # all 24 mantissa bits set, every binade
    sub = r.integers(1, 1 << 23, 2000, dtype=np.uint32)                                            # subnormals
    return np.concatenate([bits, edge, full, sub]).view(np.float32)


def test_three_bfloat16_pieces_add_up_to_the_activation():
    x = split_inputs()
    assert np.isfinite(x).all() and len(x) >= 100000
    pieces = S.split3(x)
    for p in pieces:
        assert np.isfinite(p).all()
        assert not (p.view(np.uint32) & np.uint32(0xFFFF)).any()          # a bfloat16: the low half of the F32 is zero
    total = sum(p.astype(np.float64) for p in pieces)
    x64 = x.astype(np.float64)
    scaled = x64 * 2.0 ** 133                                             # (exact: a power of two, far inside float64's range)
    fine = scaled == np.rint(scaled)                                      # x's last bit is >= 2^-133
    assert fine.sum() > 90000 and (~fine).sum() > 1000                    # both regimes are present
    assert np.array_equal(total[fine], x64[fine])
    assert (np.abs(x64 - total)[~fine] <= 2.0 ** -134).all()
    # the first piece alone is the correctly rounded bfloat16 (never further than half a bfloat16 ulp, i.e. 2^-9 relative, for normal values)
    normal = np.abs(x64) >= 2.0 ** -126
    assert (np.abs(x64 - pieces[0].astype(np.float64))[normal] <= 2.0 ** -8 * np.abs(x64)[normal]).all()


def test_rounding_is_to_nearest_even_and_never_to_infinity():
    def f(bits):
        return np.array(bits, np.uint32).view(np.float32)
    got = S.rn_bf16(f([0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x7F7FFFFF, 0xFF7F8000, 0x7F800000, 0x00008000, 0x00018000]))
    want = f([0x3F800000, 0x3F820000, 0x3F810000, 0x3F800000, 0x7F7F0000, 0xFF7F0000, 0x7F800000, 0x00000000, 0x00020000])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.isnan(S.rn_bf16(f([0x7F800001]))[0])


# ------------------------------------------------------------------------------------------------ the plan
def compilers():
    env = os.environ.get("CXX")
    return ([env] if env else []) + ["c++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_dense16_plan") / "gemm_dense16_plan_check")
    tried = []
    for cxx in compilers():
        if shutil.which(cxx) is None:
            tried.append("%s: not found" % cxx)
            continue
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "gemm_dense16_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        tried.append("%s: %s" % (cxx, r.stderr.strip()[-400:]))
    pytest.fail("no host C++ compiler built tests/gemm_dense16_plan_check.cpp:\n" + "\n".join(tried))


def arg(dtypes, T, in_f, rows, misaligned=-1):
    return "%s:%d:%d:%s:%d" % (",".join(str(d) for d in dtypes), T, in_f, ",".join(str(r) for r in rows), misaligned)


def run(exe, args):
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(args)
    res = []
    for line in out:
        d = {}
        for w in line.split(" : ")[1].split():
            k, v = w.split("=")
            d[k] = int(v)
        res.append(d)
    return res


SHAPES = [((16,), 32), ((304,), 2080), ((4096, 1024, 1024), 4096), ((128256,), 4096), ((64, 16, 16), 256), ((48,), 4096), ((14336, 14336), 4096), ((4096,), 14336),
          ((8192,), 8192), ((272, 16), 96)]
ALL_T = [1, 2, 15, 16, 17, 32, 33, 63, 64, 65, 70, 129, 256, 1000, 1024]
REQUIRED = [((16,), 32, 1), ((304,), 2080, 70), ((4096, 1024, 1024), 4096, 1024), ((128256,), 4096, 16)]


def grid():
    cases = [(dt, rows, in_f, T) for dt in (F16, BF16) for rows, in_f in SHAPES for T in ALL_T if not (rows[0] == 128256 and T > 64)]
    for rows, in_f, T in REQUIRED:
        for dt in (F16, BF16):
            assert (dt, rows, in_f, T) in cases
    return cases


def test_the_tiles_cover_every_row_and_token_exactly_once(program):
    cases = grid()
    plans = run(program, [arg([dt] * len(rows), T, in_f, rows) for dt, rows, in_f, T in cases])
    ws_bytes = None
    try:
        from ntransformer_amd import _lib
        ws_bytes = _lib.lib().ntk_gemm_dense16_workspace_bytes
    except (ImportError, OSError):
        pass
    seen_rt, seen_ntb = set(), set()
    for (dt, rows, in_f, T), p in zip(cases, plans):
        what = (dt, rows, in_f, T, p)
        assert p["status"] == 0, what
        assert p["least"] == 1 and p["most"] == 1 and p["inside"] == 1, what      # every (row, token) of every matrix: written once
        assert p["lds"] <= 163840, what
        assert p["ws"] >= p["need"], what
        assert p["planes"] == (3 if dt == BF16 else 2) and p["steps"] * 32 == in_f and p["block"] == 256, what
        assert p["ntb"] == (1 if T <= 16 else 2 if T <= 32 else 4) and p["chunks"] == (T + 63) // 64, what
        assert p["worth"] == (1 if T >= 32 else 0), what                            # the range the engine routes here (profiles/dense16_mfma.txt)
        assert p["tiles"] == sum((r + 64 * p["rt"] - 1) // (64 * p["rt"]) for r in rows), what
        assert p["grid"] == (p["tiles"] + 7) // 8 * 8 * p["chunks"], what
        if ws_bytes is not None:                                                    # the C entry point hands out the plan's size
            assert int(ws_bytes(C.c_int(in_f), C.c_int(sum(rows)), C.c_int(dt))) == p["ws"], what
        seen_rt.add(p["rt"])
        seen_ntb.add(p["ntb"])
    assert seen_rt == {1, 2, 4} and seen_ntb == {1, 2, 4}


def test_the_f16_workspace_is_the_fp16_gemms(program):
    """F16 matrices read the planes ntk_gemm_prepare_x writes: their workspace never exceeds the FP16 GEMM's for the same shape"""
    from ntransformer_amd import _lib
    L = _lib.lib()
    L.ntk_gemm_quant_workspace_bytes.restype = C.c_size_t
    for rows, in_f in SHAPES:
        need = int(L.ntk_gemm_dense16_workspace_bytes(C.c_int(in_f), C.c_int(sum(rows)), C.c_int(F16)))
        assert 0 < need <= int(L.ntk_gemm_quant_workspace_bytes(C.c_int(in_f), C.c_int(sum(rows))))
    assert int(L.ntk_gemm_dense16_workspace_bytes(C.c_int(4096), C.c_int(4096), C.c_int(int(G.DT_Q8_0)))) == 0


def test_every_refusal_is_returned(program):
    q8 = int(G.DT_Q8_0)
    cases = [
        (arg([F16], 17, 256, (24,)), E_SHAPE),                    # rows % 16
        (arg([BF16, BF16], 17, 256, (64, 8)), E_SHAPE),
        (arg([BF16], 17, 48, (64,)), E_SHAPE),                    # in_features % 32
        (arg([F16], 17, 264, (64,)), E_SHAPE),
        (arg([F16], 0, 256, (64,)), E_SHAPE),                     # outside one pass
        (arg([F16], 1025, 256, (64,)), E_SHAPE),
        (arg([F16] * 4, 17, 256, (16, 16, 16, 16)), E_SHAPE),     # more than three matrices
        (arg([q8], 17, 256, (64,)), E_DTYPE),                     # not a 16-bit dtype
        (arg([int(G.DT_F32)], 17, 256, (64,)), E_DTYPE),
        (arg([F16, BF16], 17, 256, (64, 64)), E_DTYPE),           # mixed segments
        (arg([BF16, F16, BF16], 17, 256, (64, 64, 64)), E_DTYPE),
        (arg([BF16, q8], 17, 256, (64, 64)), E_DTYPE),
    ]
    cases += [(arg([F16, F16], 17, 256, (64, 32), k), E_ALIGN) for k in range(7)]     # W0, Y0, W1, Y1, X, resid, workspace
    cases += [(arg([BF16], 1, 32, (16,), k), E_ALIGN) for k in range(5)]
    got = run(program, [a for a, _ in cases])
    for (a, want), p in zip(cases, got):
        assert p == {"status": want}, (a, p)
    assert run(program, [arg([F16, F16], 17, 256, (64, 32), -1)])[0]["status"] == 0
