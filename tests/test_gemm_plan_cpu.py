"""csrc/gemm_f16_plan.h -- the prompt GEMM's launch plan -- on the CPU (no GPU needed): a stand-alone host program (tests/gemm_plan_check.cpp, nothing
but that header) prints the plan of every shape of TABLE, and the lines must be those of tests/golden/gemm_f16_plans.txt.

That table was NOT written by the header: it was recorded from the launch code of the commit before the plan had a header of its own (a7ff896), whose
launch_gemm_f16 was patched to print every value it had chosen just before each launch (and to return instead of launching), compiled with a main()
that calls ntk_gemm_quant_f16 once per shape with pointers that are never followed; it runs without a GPU.  A plan that changes changes the bits and
the speed of the prompt pass, so a deliberate change re-records the table from the code that is being replaced, never from the code under test.

Beside the table: the forms that were retired do not come back, Q6_K takes the same K slices raw and repacked (the same sums in the same order:
identical bits), and the shapes of tests/test_gemm_f16_bits_pinned.py reach, between them, every branch of the plan."""
import os
import shutil
import subprocess

import pytest

import test_gemm_f16_bits_pinned as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLE_FILE = os.path.join(ROOT, "tests", "golden", "gemm_f16_plans.txt")
FORMATS = ["Q8_0", "Q4_0", "Q4_K", "Q5_K", "Q6_K", "Q4_K_RP", "Q5_K_RP", "Q6_K_RP"]
ALL_T = [1, 16, 17, 32, 33, 64, 65, 128, 192, 193, 256, 1024]
MODEL_8B = [(4096, (4096, 1024, 1024)), (4096, (4096,)), (4096, (14336, 14336)), (14336, (4096,)), (4096, (128256,))]
MODEL_70B = [(8192, (8192, 1024, 1024)), (8192, (8192,)), (8192, (28672, 28672)), (28672, (8192,))]
# the small and odd shapes of the GEMM tests; in = 128 / 384 / 640: whole units of Q8_0 only (NTK_E_SHAPE for the others)
SMALL = [(128, (16,)), (256, (32,)), (384, (48,)), (512, (64,)), (640, (144,)), (768, (272,)), (1024, (64, 32, 32)), (2048, (208, 208))]


def table():
    """[(format, T, in, rows, full_form)].  Not the full product: Q8_0 and Q4_K take every T on the 8B shapes and 16 / 1024 tokens on the 70B ones, the
    other formats 16 / 1024 tokens on four model shapes; full_form at the Wo shape (Q8_0, Q6_K and its repack: the LM head too); the small shapes at 5
    tokens (Q8_0, Q6_K and its repack: 20 and 200 too)"""
    out = []
    for fmt in FORMATS:
        wide = fmt in ("Q8_0", "Q6_K", "Q6_K_RP")
        if fmt in ("Q8_0", "Q4_K"):
            out += [(fmt, T, i, r, 0) for i, r in MODEL_8B for T in ALL_T] + [(fmt, T, i, r, 0) for i, r in MODEL_70B for T in (16, 1024)]
        else:
            out += [(fmt, T, i, r, 0) for i, r in (MODEL_8B[0], MODEL_8B[2], MODEL_8B[3], MODEL_70B[2]) for T in (16, 1024)]
        out += [(fmt, 5, i, r, 1) for i, r in ([MODEL_8B[1], MODEL_8B[4]] if wide else [MODEL_8B[1]])]
        out += [(fmt, T, i, r, 0) for i, r in SMALL for T in ((5, 20, 200) if wide else (5,))]
    return out


def arg(fmt, T, in_f, rows, full):
    return "%s:%d:%d:%s:%d" % (fmt, T, in_f, ",".join(str(r) for r in rows), full)


def table_args():
    return [arg(*s) for s in table()]


def compilers():
    env = os.environ.get("CXX")
    return ([env] if env else []) + ["c++", "/opt/rocm/llvm/bin/clang++", "/opt/rocm/lib/llvm/bin/clang++"]


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gemm_plan") / "gemm_plan_check")
    tried = []
    for cxx in compilers():
        if shutil.which(cxx) is None:
            tried.append("%s: not found" % cxx)
            continue
        r = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "gemm_plan_check.cpp"), "-o", exe],
                           capture_output=True, text=True)
        if r.returncode == 0:
            return exe
        tried.append("%s: %s" % (cxx, r.stderr.strip()[-400:]))
    pytest.fail("no host C++ compiler built tests/gemm_plan_check.cpp (the library could not have been built either):\n" + "\n".join(tried))


def parse(line):
    """'Q8_0 T=5 in=512 rows=64 full=0 : form=kslice rt=1 ...' -> dict (numbers as int; grid, seg as they are)"""
    head, tail = line.split(" : ")
    d = {"fmt": head.split()[0]}
    for w in head.split()[1:] + tail.split():
        k, v = w.split("=")
        if k != "seg":
            d[k] = int(v) if v.lstrip("-").isdigit() else v
    return d


def plans(exe, args):
    out = subprocess.run([exe] + args, capture_output=True, text=True, check=True).stdout.splitlines()
    assert len(out) == len(args)
    return out


@pytest.fixture(scope="module")
def table_lines(program):
    return plans(program, table_args())


def test_plans_are_the_ones_recorded_from_the_former_launch_code(table_lines):
    with open(TABLE_FILE) as f:
        want = f.read().splitlines()
    assert len(want) == len(table_lines)
    for got, rec in zip(table_lines, want):
        assert got == rec
    refused = [parse(line) for line in table_lines if "status=" in line]
    assert refused and all(p["status"] == -2 and p["fmt"] != "Q8_0" and p["in"] in (128, 384, 640) for p in refused)   # NTK_E_SHAPE: no whole unit


def test_retired_forms_do_not_come_back(table_lines):
    """Q8_0's K-slice form in units of 4 blocks (not the wide units of 8 or 16), 8 waves per workgroup; the chunk form with two workgroups per CU (80 KB
    of LDS each, not three of 53 KB)"""
    seen = 0
    for p in (parse(line) for line in table_lines if "status=" not in line):
        if p["form"] == "kslice":
            assert p["waves"] == 8 and p["block"] == 512
            if p["fmt"] == "Q8_0":
                seen += 1
                assert p["lds"] == p["per_split"] * 4 * 2 * p["ntb"] * 1024 + 8 * 16 * p["rt"] * 176
                assert p["nsplit"] * p["per_split"] * 4 * 32 == p["in"]
        if p["form"] == "chunk":
            assert p["block"] == 256 and 53 * 1024 < p["lds"] <= 80 * 1024
    assert seen >= 20


def test_q6_k_takes_the_same_slices_raw_and_repacked(table_lines):
    by = {}
    for p in (parse(line) for line in table_lines):
        by[(p["fmt"], p["T"], p["in"], p["rows"], p["full"])] = p
    n = 0
    for (fmt, T, i, r, full), raw in by.items():
        if fmt != "Q6_K":
            continue
        rp = by[("Q6_K_RP", T, i, r, full)]
        for k in ("status", "form", "rt", "ntb", "nsplit", "per_split", "jobs", "tiles"):
            assert raw.get(k) == rp.get(k), (T, i, r, full, k)
        n += 1
    assert n >= 30


def test_the_pinned_bits_cases_reach_every_branch_of_the_plan(program):
    args, owner = [], []
    for c in B.CASES:
        for T, full in B.passes(c):
            args.append(arg(c["fmt"], T, c["in_f"], c["rows"], full))
            owner.append(c)
    ps = [parse(line) for line in plans(program, args)]
    assert all("form" in p for p in ps)
    for fmt in FORMATS:                                     # each format in each of the three forms
        assert {p["form"] for p in ps if p["fmt"] == fmt} == {"kslice", "small", "chunk"}, fmt
    ks = [p for p in ps if p["form"] == "kslice"]
    ch = [p for p in ps if p["form"] == "chunk"]
    assert {p["ntb"] for p in ks} == {1, 2} and {p["rt"] for p in ks} == {1, 2}
    assert any(p["nsplit"] == 1 for p in ks) and any(p["nsplit"] > 1 for p in ks) and any(p["jobs"] > 1 for p in ks)
    assert {p["ntb"] for p in ps if p["form"] == "small"} == {1, 2}
    assert {p["cw"] for p in ch} == {1, 2} and {p["rt"] for p in ch} == {1, 2} and {p["pf"] for p in ch} == {0, 1}
    assert any(p["nsplit"] == 1 for p in ch) and any(p["nsplit"] > 1 for p in ch)
    assert {p["al"] for p in ch} == {0, 1} and {p["al"] for p in ps if p["form"] == "small"} == {0, 1}
    assert any(c["T"] > B.PASS for c in B.CASES)            # a call of two passes
    for form in ("kslice", "small", "chunk"):               # three matrices sharing X, once per form
        assert any(p["form"] == form and len(c["rows"]) == 3 for p, c in zip(ps, owner)), form
    for kind, forms in (("resid", {"kslice", "small", "chunk"}), ("norm", {"kslice", "chunk"}), ("silu", {"kslice", "chunk"})):
        got = {(p["form"], p["nsplit"] > 1) for p, c in zip(ps, owner) if c["kind"] == kind}
        assert {f for f, _ in got} == forms and {s for _, s in got} == {False, True}, kind   # with the K splits left to the consumer, and without
    assert all(p["form"] == "chunk" for p, c in zip(ps, owner) if c["kind"] == "full")
