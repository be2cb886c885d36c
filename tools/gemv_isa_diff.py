#!/usr/bin/env python3
"""Did a change of the sources change the kernels?  Compiles one device source of ntransformer_amd/csrc (--source, default gemv.hip: the decode
GEMV) of git revision <rev> and of the working tree to gfx950 assembly with the Makefile's flags -- the per-file extra flags included (the FLAGS_<stem>
lines of each tree's csrc/Makefile) -- and compares them kernel symbol by kernel symbol (no GPU needed, ~20 s per build of gemv.hip): the
instruction streams with labels renumbered and comments dropped, and the compiler's figures per kernel (VGPRs, spilled VGPRs, private segment,
occupancy, static LDS, SGPRs, code length).  Prints the list of symbols and per kernel "identical" or the figures and the first differing lines.

    python tools/gemv_isa_diff.py f5f1f26 > profiles/gemv_stages_isa.txt
    python tools/gemv_isa_diff.py f5f1f26 --source attention_q8.hip
"""
import argparse
import difflib
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "ntransformer_amd/csrc"
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -fvisibility=hidden -Wall -Wno-unused-function -Wno-unused-variable"   # csrc/Makefile HIPFLAGS
FIGURES = [("vgprs", r"; NumVgprs: (\d+)"), ("spilled_vgprs", None), ("private_segment", r"; ScratchSize: (\d+)"), ("occupancy", r"; Occupancy: (\d+)"),
           ("static_lds", r"; LDSByteSize: (\d+)"), ("sgprs", r"; TotalNumSgprs: (\d+)"), ("code_bytes", r"; codeLenInByte = (\d+)")]
BOUNDED = {"vgprs": "max", "spilled_vgprs": "max", "private_segment": "max", "occupancy": "min", "static_lds": "eq"}   # the rest is reported only


def assembly(tree, hipcc, extra, source):
    """(assembly text, flags used): HIPFLAGS + the tree's own `FLAGS_<stem> := ...` line of csrc/Makefile for this source + extra"""
    with open(os.path.join(tree, CSRC, "Makefile")) as f:
        own = re.search(r"^FLAGS_%s\s*:=\s*(.*)$" % re.escape(os.path.splitext(source)[0]), f.read(), re.M)
    extra = " ".join(x for x in (own.group(1).strip() if own else "", extra) if x)
    out = tempfile.NamedTemporaryFile(suffix=".s", delete=False).name
    cmd = [hipcc] + FLAGS.split() + extra.split() + ["-S", "--cuda-device-only", source, "-o", out]
    subprocess.run(cmd, cwd=os.path.join(tree, CSRC), check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        text = f.read()
    os.unlink(out)
    return text, extra


def kernels(text):
    """{symbol: (normalised instruction lines, figures)} of every kernel of an assembly file"""
    names = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    spills = dict(re.findall(r"\.symbol:\s+(\S+)\.kd\n\s+\.uniform_work_group_size:.*\n\s+\.uses_dynamic_stack:.*\n\s+\.vgpr_count:.*\n\s+\.vgpr_spill_count:\s+(\d+)", text))
    if len(spills) != len(names):   # (a metadata layout this pattern does not know: take the counts one by one)
        spills = dict(zip(re.findall(r"\.symbol:\s+(\S+)\.kd", text), re.findall(r"\.vgpr_spill_count:\s+(\d+)", text)))
    out = {}
    for name in names:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\s*\.section\s+\.rodata(.*?)(?:; -- Begin function|\Z)" % re.escape(name), text, re.M | re.S)
        body, tail = m.group(1), m.group(2)
        lines = []
        for ln in body.split("\n"):
            ln = re.sub(r";.*", "", ln).strip()
            ln = re.sub(r"\.L(BB|tmp|func_\w+)\d+(_\d+)?", lambda k: ".L%s%s" % (k.group(1), k.group(2) or ""), ln)
            if ln:
                lines.append(ln)
        fig = {}
        for key, pat in FIGURES:
            fig[key] = int(spills[name]) if pat is None else int(re.search(pat, tail).group(1))
        out[name] = (lines, fig)
    return out


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        res = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, res))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("rev")
    ap.add_argument("--hipcc", default="/opt/rocm/bin/hipcc")
    ap.add_argument("--flags", default="", help="extra flags for both builds (e.g. -DNTK_GEMV_TRACE)")
    ap.add_argument("--source", default="gemv.hip", help="the device source of ntransformer_amd/csrc to compare (sources.mk)")
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        tar = subprocess.run(["git", "archive", a.rev, CSRC, "include"], cwd=ROOT, check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=tar, check=True)
        old = kernels(assembly(tmp, a.hipcc, a.flags, a.source)[0])
    text, extra = assembly(ROOT, a.hipcc, a.flags, a.source)
    new = kernels(text)
    rev = subprocess.run(["git", "rev-parse", "--short", a.rev], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    nice = demangle(sorted(set(old) | set(new)))
    print("# %s -> gfx950 assembly, %s against the working tree; flags: %s %s" % (a.source, rev, FLAGS, extra))
    print("# kernels: %d at %s, %d now; symbols only at %s: %s; only now: %s" % (len(old), rev, len(new), rev, sorted(set(old) - set(new)) or "none",
                                                                               sorted(set(new) - set(old)) or "none"))
    bad = 0
    for name in sorted(old, key=lambda n: nice[n]):
        lo, fo = old[name]
        line = "  ".join("%s=%d" % (k, fo[k]) for k, _ in FIGURES)
        if name not in new:
            print("%s\n    GONE    %s" % (nice[name], line))
            bad += 1
            continue
        ln, fn = new[name]
        if lo == ln and fo == fn:
            print("%s\n    identical    %s" % (nice[name], line))
            continue
        worse = [k for k, how in BOUNDED.items() if (how == "max" and fn[k] > fo[k]) or (how == "min" and fn[k] < fo[k]) or (how == "eq" and fn[k] != fo[k])]
        bad += bool(worse)
        d = [x for x in difflib.unified_diff(lo, ln, lineterm="", n=0) if not x.startswith(("---", "+++", "@@"))]
        print("%s\n    DIFFERENT%s    %d of %d lines\n    was  %s\n    now  %s" % (nice[name], "  WORSE: " + ",".join(worse) if worse else "", len(d), len(lo), line,
                                                                                   "  ".join("%s=%d" % (k, fn[k]) for k, _ in FIGURES)))
        for x in d[:12]:
            print("        " + x)
    same = sum(1 for n in old if n in new and old[n] == new[n])
    print("# %d of %d kernels identical; %d gone or worse in a bounded figure" % (same, len(old), bad))
    return 1 if bad or set(old) != set(new) else 0


if __name__ == "__main__":
    sys.exit(main())
