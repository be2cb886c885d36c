"""The packed prompt pass on the CPU (no GPU): its entry points are declared and exported, the host-only argument checks of nt_engine_forward_batch
(nt_forward_batch_validate) and of the two segment launchers (ntk_kv_segments_validate) accept and refuse what the headers say, and the numpy
reference the GPU tests compare with -- the oracle's attention_prefill, segment by segment (segments_reference below, imported by
tests/test_attention_segments_gpu.py) -- is itself checked against a direct float64 masked softmax."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from ntransformer_amd import _lib, ops
from ntransformer_amd import engine as E
from oracle import oracle as O

OK, E_SHAPE, E_NULL = 0, -2, -5
NEW = {"ntransformer.h": ("nt_engine_forward_batch", "nt_forward_batch_validate"),
       "ntk_engine.h": ("ntk_rope_kv_store_segments", "ntk_attention_prefill_segments", "ntk_kv_segments_validate")}


@pytest.mark.parametrize("header", sorted(NEW))
def test_the_new_entry_points_are_declared_and_exported(header):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    L = _lib.lib()
    exported = None
    if shutil.which("nm"):
        out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True).stdout
        exported = {l.split()[-1] for l in out.splitlines() if " T " in l}
    for name in NEW[header]:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name), name
        assert exported is None or name in exported, name


SEQ, CTX = 16, 256
FORWARD_BATCH_CASES = [
    # (what, slots, lens, starts, n or None, expected)
    ("one segment", [0], [5], [0], None, OK),
    ("one segment filling the context", [3], [CTX], [0], None, OK),
    ("16 segments, lengths summing exactly to the context", list(range(16)), [16] * 16, [CTX - 16] * 16, None, OK),
    ("16 segments in another slot order, ragged", list(range(15, -1, -1)), list(range(1, 17)), list(range(16)), None, OK),
    ("a slot twice", [0, 1, 0], [1, 2, 3], [0, 0, 0], None, E_SHAPE),
    ("a slot equal to `sequences`", [0, SEQ], [1, 2], [0, 0], None, E_SHAPE),
    ("a negative slot", [-1], [1], [0], None, E_SHAPE),
    ("a length of 0", [0, 1], [4, 0], [0, 0], None, E_SHAPE),
    ("a negative start", [0, 1], [4, 1], [0, -1], None, E_SHAPE),
    ("start + length == max_seq", [0, 1], [4, 6], [0, CTX - 6], None, OK),
    ("start + length == max_seq + 1", [0, 1], [4, 6], [0, CTX - 5], None, E_SHAPE),
    ("a sum equal to max_seq + 1", [0, 1, 2], [CTX - 10, 6, 5], [0, 0, 0], None, E_SHAPE),
    ("n = 0", [0], [1], [0], 0, E_SHAPE),
    ("n = sequences + 1", list(range(16)) + [0], [1] * 17, [0] * 17, 17, E_SHAPE),
]


@pytest.mark.parametrize("what,slots,lens,starts,n,want", FORWARD_BATCH_CASES, ids=[c[0] for c in FORWARD_BATCH_CASES])
def test_forward_batch_validate(what, slots, lens, starts, n, want):
    assert E.forward_batch_validate(slots, lens, starts, SEQ, CTX, n=n) == want


def test_forward_batch_validate_fewer_slots_and_null():
    """n is held to the engine's `sequences`, not to 16; NULL arrays: NTK_E_NULL"""
    assert E.forward_batch_validate([0, 1, 2], [1, 1, 1], [0, 0, 0], 3, CTX) == OK
    assert E.forward_batch_validate([0, 1, 2, 3], [1, 1, 1, 1], [0, 0, 0, 0], 3, CTX) == E_SHAPE
    assert E._bind().nt_forward_batch_validate(None, None, None, 1, SEQ, CTX) == E_NULL


K = [0x1000 * (s + 1) for s in range(17)]          # stand-ins for device addresses: the check is host only and never follows them
V = [0x100000 + 0x1000 * (s + 1) for s in range(17)]
A = [(1, 0), (1, 37), (15, 0), (16, 64), (17, 5), (63, 1), (64, 0), (65, 127), (70, 186)]   # the GPU test's set A: 312 rows
SEGMENT_CASES = [
    # (what, segments, kwargs of ops.kv_segments, total_rows, max_seq, expected)
    ("one segment", [(5, 0)], {}, 5, CTX, OK),
    ("set A", A, {}, 312, CTX, OK),
    ("16 segments", [(n, n - 1) for n in range(1, 17)], {}, 136, CTX, OK),
    ("n_seg = 0", [(5, 0)], dict(n_seg=0), 5, CTX, E_SHAPE),
    ("n_seg = 17", [(1, 0)] * 16, dict(n_seg=17), 17, CTX, E_SHAPE),
    ("a gap in row0", [(5, 0), (3, 0)], dict(row0=[0, 6]), 9, CTX, E_SHAPE),
    ("overlapping row0", [(5, 0), (3, 0)], dict(row0=[0, 4]), 7, CTX, E_SHAPE),
    ("row0[0] != 0", [(5, 0), (3, 0)], dict(row0=[1, 6]), 9, CTX, E_SHAPE),
    ("a total that is not the sum of the lengths", [(5, 0), (3, 0)], {}, 9, CTX, E_SHAPE),
    ("a length of 0", [(5, 0), (0, 0)], {}, 5, CTX, E_SHAPE),
    ("a negative start", [(5, -1)], {}, 5, CTX, E_SHAPE),
    ("start + length == max_seq", [(5, CTX - 5)], {}, 5, CTX, OK),
    ("start + length == max_seq + 1", [(5, CTX - 4)], {}, 5, CTX, E_SHAPE),
    ("two segments naming the same k cache", [(5, 0), (3, 0), (2, 0)], dict(k_caches=[K[0], K[1], K[0]]), 10, CTX, E_SHAPE),
    ("a NULL k cache", [(5, 0), (3, 0)], dict(k_caches=[K[0], None]), 8, CTX, E_NULL),
    ("a NULL v cache", [(5, 0), (3, 0)], dict(v_caches=[None, V[1]]), 8, CTX, E_NULL),
]


@pytest.mark.parametrize("what,segments,kw,total,max_seq,want", SEGMENT_CASES, ids=[c[0] for c in SEGMENT_CASES])
def test_kv_segments_validate(what, segments, kw, total, max_seq, want):
    kw = dict(dict(k_caches=K, v_caches=V), **kw)
    assert ops.kv_segments_validate(ops.kv_segments(segments, **kw), total, max_seq) == want


def test_kv_segments_validate_null_descriptor_and_pointers_past_n_seg():
    assert ops.kv_segments_validate(None, 1, CTX) == E_NULL
    d = ops.kv_segments([(5, 0), (3, 0)], K, V)          # entries 2 .. 15 stay NULL: ignored
    assert ops.kv_segments_validate(d, 8, CTX) == OK


def segments_reference(Q, segments, caches, nh, nkv, hd, max_seq, scale):
    """The reference of ntk_attention_prefill_segments: the oracle's attention_prefill on every segment alone -- its rows of Q, its (K, V) cache image
    (uint16 halves [max_seq * nkv * hd]), its start position -- concatenated in row order.  Q [rows][nh * hd]."""
    out, row = [], 0
    for (n, start), (kc, vc) in zip(segments, caches):
        out.append(O.attention_prefill(Q[row:row + n].reshape(-1), kc, vc, n, start, nh, nkv, hd, max_seq, scale).reshape(n, nh * hd))
        row += n
    return np.concatenate(out)


def test_the_segment_reference_is_a_masked_softmax_per_segment():
    """segments_reference against float64 softmax(scale q . K^T over rows 0 .. start + t of the segment's OWN cache) V, one small case: three segments
    (a single row at a non-zero start, a chunk, a prompt from 0), GQA 2, rows past each segment's last key NaN."""
    nh, nkv, hd, max_seq = 4, 2, 16, 24
    segments = [(1, 7), (5, 3), (6, 0)]
    r = np.random.Generator(np.random.Philox(key=[20261019, 1]))
    rows = sum(n for n, _ in segments)
    Q = r.standard_normal((rows, nh * hd)).astype(np.float32)
    caches = []
    for n, start in segments:
        kc, vc = (np.full(max_seq * nkv * hd, 0x7E00, np.uint16) for _ in range(2))
        kc[: (start + n) * nkv * hd] = r.standard_normal((start + n) * nkv * hd).astype(np.float16).view(np.uint16)
        vc[: (start + n) * nkv * hd] = r.standard_normal((start + n) * nkv * hd).astype(np.float16).view(np.uint16)
        caches.append((kc, vc))
    scale = float(1 / np.sqrt(hd))
    got = segments_reference(Q, segments, caches, nh, nkv, hd, max_seq, scale)
    assert got.shape == (rows, nh * hd) and np.isfinite(got).all()
    row = 0
    for (n, start), (kc, vc) in zip(segments, caches):
        Kf = kc.view(np.float16).astype(np.float64).reshape(max_seq, nkv, hd)
        Vf = vc.view(np.float16).astype(np.float64).reshape(max_seq, nkv, hd)
        for t in range(n):
            keys = start + t + 1
            for h in range(nh):
                g = h // (nh // nkv)
                s = scale * (Kf[:keys, g] @ Q[row + t, h * hd:(h + 1) * hd].astype(np.float64))
                p = np.exp(s - s.max())
                want = (p / p.sum()) @ Vf[:keys, g]
                assert np.abs(got[row + t, h * hd:(h + 1) * hd] - want).max() <= 2e-6, (n, start, t, h)
        row += n
