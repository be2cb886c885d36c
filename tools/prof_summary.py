#!/usr/bin/env python3
"""Summarise a rocprofv3 --kernel-trace run of bench.py (rocpd sqlite database or kernel_trace CSV) per kernel
for the DECODE window only: dispatches after the last prefill attention launch.  bench.py's `roofline` numbers are
measured over decode tokens, so this is the slice of the trace they must agree with.
usage: python tools/prof_summary.py <results.db> [--bytes-per-token N] > profiles/<name>.txt"""
import argparse
import collections
import sqlite3
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("db")
    ap.add_argument("--gemv-bytes-per-token", type=float, default=7_973_699_584.0, help="bytes the GEMV launches of one token stream")
    ap.add_argument("--json", default=None, help="merge {key: GEMV launches of this trace} into this file (profiles/trace_gemv.json, read back by bench.py as frac_trace)")
    ap.add_argument("--key", default=None, help="workload key of --json: <model>_<mix>[_ctx<prompt tokens>], e.g. 8b_q8_0")
    ap.add_argument("--file", default="", help="name of the committed summary this trace becomes (recorded beside the numbers)")
    a = ap.parse_args()
    db = sqlite3.connect(a.db)
    rows = db.execute("select name, start, end, grid_x, workgroup_x, vgpr_count, lds_size from kernels order by start").fetchall()
    last_prefill = max((i for i, r in enumerate(rows) if "attention_kernel<" in r[0]), default=-1)
    dec = rows[last_prefill + 1:]
    # drop everything up to the end of prefill's token (final norm + LM head + first argmax): start at first fused attention
    first = next((i for i, r in enumerate(dec) if "attention_decode_" in r[0]), 0)   # (single pass, split walk or the matrix-core form)
    first_embed = max((i for i in range(first) if "embed_rows" in dec[i][0]), default=0)
    dec = [r for r in dec[first_embed:] if "sclk_" not in r[0]]   # (the clock probes of bench.py are not part of the token)
    n_tokens = sum(1 for r in dec if "embed_rows" in r[0])
    stats = collections.OrderedDict()
    for name, s, e, gx, wx, vg, lds in dec:
        short = name.split("(")[0].replace("void ", "")
        st = stats.setdefault(short, [0, 0.0, set()])
        st[0] += 1
        st[1] += (e - s) / 1e3
        st[2].add((gx // max(wx, 1), wx, vg, lds))
    span_us = (dec[-1][2] - dec[0][1]) / 1e3 if dec else 0.0
    busy = sum(v[1] for v in stats.values())
    print("decode window: %d kernel dispatches, %d tokens, span %.1f us (%.1f us/token), kernel-busy %.1f us (%.1f%%)"
          % (len(dec), n_tokens, span_us, span_us / max(n_tokens, 1), busy, 100 * busy / max(span_us, 1e-9)))
    print("%-48s %8s %12s %10s %7s" % ("kernel", "calls", "total_us", "avg_us", "share"))
    for k, (c, t, shapes) in sorted(stats.items(), key=lambda kv: -kv[1][1]):
        print("%-48s %8d %12.1f %10.2f %6.1f%%" % (k, c, t, t / c, 100 * t / busy))
    # every form: plain, integer-activation (xi), two-format (pair), matrix-core (rp), lane-major Q8_0 (q8l)
    is_gemv = lambda k: "gemv_quant_" in k or "rp_gemv_kernel" in k or "gemv_q8l_kernel" in k
    g = [v for k, v in stats.items() if is_gemv(k)]
    if g and n_tokens:
        c, t = sum(v[0] for v in g), sum(v[1] for v in g)
        per_launch = a.gemv_bytes_per_token * n_tokens / c
        print("\ngemv launches (gemv_quant_* + rp_gemv_kernel + gemv_q8l_kernel) pooled: %.1f launches/token, avg %.2f us, algorithmic %.1f MB/launch -> %.1f GB/s = %.1f%% of 8 TB/s"
              % (c / n_tokens, t / c, per_launch / 1e6, per_launch / (t / c * 1e-6) / 1e9, per_launch / (t / c * 1e-6) / 8e12 * 100))
        print("kernel time per token: %.1f us all kernels, %.1f us GEMV launches" % (busy / n_tokens, t / n_tokens))
        # the GEMV launches of a token by KIND, from their order inside the token (fused path: Q|K|V, Wo, gate|up, down per layer, the LM head last):
        # average duration per kind -- bench.py pairs them with the kinds' bytes and fits t = fixed + bytes / rate (roofline.launch_model)
        kinds = {}
        tok_runs, cur = [], None
        for r in dec:
            if "embed_rows" in r[0]:
                cur = []
                tok_runs.append(cur)
            elif cur is not None and is_gemv(r[0]):
                cur.append((r[2] - r[1]) / 1e3)
        full = [t_ for t_ in tok_runs if len(t_) == round(c / n_tokens) and (len(t_) - 1) % 4 == 0]
        if full:
            names = ("qkv", "wo", "gate_up", "down")
            acc = collections.defaultdict(list)
            for t_ in full:
                for i, us in enumerate(t_[:-1]):
                    acc[names[i % 4]].append(us)
                acc["lm_head"].append(t_[-1])
            kinds = {k: {"avg_us": round(sum(v) / len(v), 3), "calls": len(v)} for k, v in acc.items()}
            print("gemv launches by kind (order inside the token): " + ", ".join("%s %.2f us" % (k, kinds[k]["avg_us"]) for k in names + ("lm_head",)))
        if a.json and a.key:
            import json
            import os
            d = json.load(open(a.json)) if os.path.exists(a.json) else {}
            d[a.key] = {"avg_us": round(t / c, 3), "launches_per_token": round(c / n_tokens, 2), "bytes_per_launch": int(per_launch),
                        "frac": round(per_launch / (t / c * 1e-6) / 8e12, 4), "kernel_us_per_token": round(busy / n_tokens, 1), "tokens": n_tokens,
                        "file": a.file, "kinds": kinds}
            json.dump(d, open(a.json, "w"), indent=1, sort_keys=True)
    # per launch geometry of the GEMV (grid in workgroups, block, vgprs, lds): one line per distinct shape
    byshape = collections.defaultdict(lambda: [0, 0.0])
    for name, s, e, gx, wx, vg, lds in dec:
        if is_gemv(name):
            k = (name.split("(")[0].replace("void ", "").replace("ntk::", "")[:34], gx // max(wx, 1), wx, vg, lds)
            byshape[k][0] += 1
            byshape[k][1] += (e - s) / 1e3
    print("\ngemv launches by geometry (workgroups, threads, vgprs, lds bytes): calls, avg us")
    for k, (c, t) in sorted(byshape.items(), key=lambda kv: -kv[1][1]):
        print("  %-70s %6d %9.2f" % (k, c, t / c))


if __name__ == "__main__":
    main()
