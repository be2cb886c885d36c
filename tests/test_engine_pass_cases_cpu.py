"""CPU test of the case list of tests/test_engine_pass_bits_pinned.py: its models reach the LM-head workspace branch they are there for
(Model::lm_head_workspace allocates when the head needs more than the load-time GEMM workspace -- Model::alloc_buffers' shapes), and every case's
calls stay inside the context and the slots it asks for.  No GPU needed: ntk_gemm_quant_workspace_bytes is host arithmetic."""
import ctypes as C

from ntransformer_amd import _lib
import test_engine_pass_bits_pinned as P


def _workspaces(s):
    """(load-time GEMM workspace, the LM head's need) of shape s"""
    L = _lib.lib()
    L.ntk_gemm_quant_workspace_bytes.restype = C.c_size_t
    ws = lambda in_f, out_f: int(L.ntk_gemm_quant_workspace_bytes(C.c_int(in_f), C.c_int(out_f)))
    hd = s.hidden // s.heads
    H, I, q, kv = s.hidden, s.inter, s.heads * hd, s.kv_heads * hd
    load = max(ws(i, o) for i, o in ((H, q + 2 * kv), (H, q), (H, kv), (q, H), (H, 2 * I), (H, I), (I, H)))
    return load, ws(H, s.vocab)


def test_only_bigv_outgrows_the_load_time_workspace():
    for name, s in P.SHAPES.items():
        load, head = _workspaces(s)
        assert (head > load) == (name == "bigv"), (name, load, head)


def test_cases_stay_inside_context_and_slots():
    assert len(P.CASES) >= 40
    for c in P.CASES:
        nslots = int(c["opts"].get("sequences", 1))
        pos = {}
        for st in c["steps"]:
            if st[0] == "forward": rows = [(0, st[2], st[1])]
            elif st[0] == "prefill": rows = [(st[1], 0, st[2])]
            elif st[0] == "score": rows = [(0, 0, st[1])]
            elif st[0] in ("decode_batch", "sample"): rows = [(s, pos[s], 1) for s in st[1]]
            elif st[0] == "forward_batch": rows = list(zip(st[1], st[3], st[2]))
            else: rows = []
            for slot, p0, n in rows:
                assert 0 <= slot < nslots and n >= 1 and p0 + n + 2 <= P.CTX, c["id"]     # (+ 2: the fused steps behind the case)
                if st[0] == "forward_batch": assert p0 == pos.get(slot, 0), c["id"]      # a segment continues its slot
                pos[slot] = max(pos.get(slot, 0), p0 + n)
