"""The row form of the routed expert FFN (csrc/moe_row.hip) through the C ABI: ntk_moe_ffn_row against ntk_moe_route -> ntk_moe_gate_up -> ntk_moe_down at
T = 1 on the same inputs BIT FOR BIT (y separate from resid and in place; the ids, w and act sections), and against a float64 routed FFN over the exactly
dequantised weights (gguf.dequantize) at tests/test_moe_gpu.py's GEMV bar.  Logits are exact integers whatever the summation order (xn is 1 in column 0 and 2
in the last, the router zero elsewhere); "tie": two equal logits at the K-th place, "nan": the best expert's logit is a NaN.  The workspace outside ids, w, act
and the E logits keeps its poison, as do the guards behind y; a repeat gives the same bits; every refusal returns its code over a poisoned y."""
import zlib

import numpy as np
import pytest

from moe_ref import select_experts, tol_for
from ntransformer_amd import _lib, gguf as G, ops
from ntransformer_amd.ops import DeviceBuffer as DB
from test_moe_gpu import POISON_F, TYPES, Out, bits

pytestmark = pytest.mark.gpu
# name: gate, up, down types, hidden, inter, E, K -- two units per row; 65 units and ragged row blocks; 210-byte rows at even addresses; the largest counts
SHAPES = {"q8-64-e1": ("Q8_0", "Q8_0", "Q8_0", 64, 96, 1, 1), "q8-64-e5": ("Q8_0", "Q8_0", "Q8_0", 64, 96, 5, 5),
          "q8-2080": ("Q8_0", "Q8_0", "Q8_0", 2080, 96, 130, 8), "k-256": ("Q4_K", "Q6_K", "Q6_K", 256, 256, 8, 2),
          "k-512": ("Q6_K", "Q4_K", "Q4_K", 512, 768, 256, 16)}
CASES = [(n, "plain") for n in SHAPES] + [("q8-2080", "tie"), ("k-256", "nan")]
DISTINCT = 16          # experts generated per tensor; the rest repeat them (256 experts of 512 x 768 would take seconds to draw)


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


_cases = {}


def case(name, variant):
    if (name, variant) in _cases:
        return _cases[(name, variant)]
    g, u, d, H, I, E, K = SHAPES[name]
    r = np.random.Generator(np.random.Philox(key=[20261126, zlib.crc32(name.encode())]))
    W = {}
    for n, t, rows, cols in (("g", g, I, H), ("u", u, I, H), ("d", d, H, I)):
        base = np.frombuffer(G.synth_tensor(r, TYPES[t], min(E, DISTINCT) * rows, cols), np.uint8)
        W[n] = np.tile(base, E // DISTINCT + 1)[:E * rows * G.row_bytes(TYPES[t], cols)]
    xn = r.standard_normal(H).astype(np.float32)
    xn[0], xn[H - 1] = 1.0, 2.0
    router = np.zeros((E, H), np.float32)
    router[:, 0] = 3.0 * (r.permutation(E) - E // 2)
    router[:, H - 1] = r.integers(0, 2, E)
    order = select_experts(router[:, 0] + 2.0 * router[:, H - 1], E)          # every expert, best first
    if variant == "tie":
        router[order[K]] = router[order[K - 1]]          # the (K + 1)-th takes the K-th's logit
    if variant == "nan":
        router[order[0], 1] = np.nan
    logits = router[:, 0] + 2.0 * router[:, H - 1]
    logits[np.isnan(router).any(1)] = np.nan
    ranked = np.where(np.isnan(logits), -np.inf, logits)
    ids = select_experts(ranked, K)
    if variant == "tie":
        assert ranked[order[K]] == ranked[order[K - 1]] and min(order[K], order[K - 1]) in ids and max(order[K], order[K - 1]) not in ids
    if variant == "nan":
        assert order[0] not in ids
    resid = r.standard_normal(H).astype(np.float32)
    # the float64 reference over the exactly dequantised weights
    sel = ranked[ids].astype(np.float64)
    w64 = np.exp(sel - sel.max())
    w64 /= w64.sum()
    x64, y64 = xn.astype(np.float64), resid.astype(np.float64)

    def deq(n, t, e, rows, cols):
        nb = rows * G.row_bytes(TYPES[t], cols)
        return G.dequantize(W[n][e * nb:(e + 1) * nb], TYPES[t], rows * cols).astype(np.float64).reshape(rows, cols)
    for k, e in enumerate(int(i) for i in ids):
        gv, uv = deq("g", g, e, I, H) @ x64, deq("u", u, e, I, H) @ x64
        y64 = y64 + w64[k] * (deq("d", d, e, H, I) @ (gv / (1.0 + np.exp(-gv)) * uv))
    dt = {n: G.GGML_TO_DT[TYPES[t]] for n, t in (("g", g), ("u", u), ("d", d))}
    off, total = ops.moe_workspace_layout(1, E, K, I, H)
    c = dict(H=H, I=I, E=E, K=K, dt=dt, ids=ids, y64=y64, resid=resid, off=off, total=total, dev={n: DB.from_numpy(W[n]) for n in W},
             xn=DB.from_numpy(xn), router=DB.from_numpy(router), dres=DB.from_numpy(resid))
    _cases[(name, variant)] = c
    return c


def poisoned_ws(c):
    return DB.from_numpy(np.full(c["total"] // 4, POISON_F, np.float32))


def three_launches(c, y_ptr, resid_ptr, ws):
    H, I, E, K, o = c["H"], c["I"], c["E"], c["K"], c["off"]
    ops.moe_route(c["xn"], c["router"], 1, H, E, K, ws.at(o["ids"]), ws.at(o["w"]), ws.at(o["offsets"]), ws.at(o["pairs"]))
    ops.moe_gate_up(ws.at(o["act"]), c["xn"], c["dev"]["g"], c["dt"]["g"], c["dev"]["u"], c["dt"]["u"], ws.at(o["offsets"]), ws.at(o["pairs"]), 1, H, I, E, K)
    ops.moe_down(y_ptr, resid_ptr, ws.at(o["act"]), c["dev"]["d"], c["dt"]["d"], ws.at(o["ids"]), ws.at(o["w"]), ws.at(o["offsets"]), ws.at(o["pairs"]),
                 ws.at(o["part"]), 1, H, I, E, K)


def row_form(c, y_ptr, resid_ptr, ws):
    ops.moe_ffn_row(y_ptr, resid_ptr, c["xn"], c["router"], c["dev"]["g"], c["dt"]["g"], c["dev"]["u"], c["dt"]["u"], c["dev"]["d"], c["dt"]["d"], c["H"],
                    c["I"], c["E"], c["K"], ws, c["total"])


def run(c, launch, alias):
    """(y, the workspace's words) of one form"""
    ws, y = poisoned_ws(c), Out(c["H"], np.float32)
    if alias:
        y.dev.upload(c["resid"])
    launch(c, y.ptr, y.ptr if alias else c["dres"], ws)
    got = y.read(), ws.numpy(np.uint32)
    ws.free(); y.dev.free()
    return got


@pytest.mark.parametrize("name,variant", CASES)
def test_row_form_has_the_bits_of_the_three_launches(name, variant):
    c = case(name, variant)
    H, I, E, K, o = c["H"], c["I"], c["E"], c["K"], c["off"]
    want_y, want_ws = run(c, three_launches, False)
    sec = lambda words, s, n: words[o[s] // 4:o[s] // 4 + n]
    assert np.array_equal(sec(want_ws, "ids", K).view(np.int32), c["ids"])          # the baseline routes as the reference does
    err, bar = float(np.abs(want_y.astype(np.float64) - c["y64"]).max()), tol_for(c["y64"], I)
    assert err <= bar, ("three launches", err, bar)
    written = np.zeros(c["total"] // 4, bool)          # what the row form may write: ids, w, act, the E logits
    for s, n in (("ids", K), ("w", K), ("act", K * I), ("part", E)):
        written[o[s] // 4:o[s] // 4 + n] = True
    for alias in (False, True, False):          # (the third: a second launch of the same form gives the same bits)
        y, ws = run(c, row_form, alias)
        assert np.array_equal(bits(y), bits(want_y)), (alias, float(np.abs(y - want_y).max()))
        for s, n in (("ids", K), ("w", K), ("act", K * I)):
            assert np.array_equal(sec(ws, s, n), sec(want_ws, s, n)), (s, alias)
        assert np.all(ws[~written] == bits(np.full(1, POISON_F))[0]), "wrote outside its sections"
        err = float(np.abs(y.astype(np.float64) - c["y64"]).max())
        assert err <= bar, ("row form", err, bar)
    assert np.array_equal(bits(c["dres"].numpy(np.float32, H)), bits(c["resid"]))


def test_refusals_leave_y_untouched():
    c = case("q8-64-e5", "plain")
    L, H, I, E, K = _lib.lib(), c["H"], c["I"], c["E"], c["K"]
    ws, y = poisoned_ws(c), Out(H, np.float32)
    q8 = G.DT_Q8_0

    def call(yy=y.ptr, r=c["dres"].ptr, x=c["xn"].ptr, rt=c["router"].ptr, g=c["dev"]["g"].ptr, dg=q8, u=c["dev"]["u"].ptr, du=q8, d=c["dev"]["d"].ptr, dd=q8,
             H=H, I=I, E=E, K=K, w=ws.ptr, wb=c["total"]):
        return L.ntk_moe_ffn_row(yy, r, x, rt, g, dg, u, du, d, dd, H, I, E, K, w, wb, None)
    NULL, SHAPE, DTYPE, ALIGN = -5, -2, -1, -4
    calls = [(call(yy=None), NULL), (call(r=None), NULL), (call(x=None), NULL), (call(rt=None), NULL), (call(g=None), NULL), (call(u=None), NULL),
             (call(d=None), NULL), (call(w=None), NULL),
             (call(dg=G.DT_F16), DTYPE), (call(du=G.DT_Q4_0), DTYPE), (call(dd=G.DT_Q5_K), DTYPE),
             (call(K=6), SHAPE), (call(E=257), SHAPE), (call(K=0), SHAPE), (call(K=17, E=32), SHAPE), (call(H=48), SHAPE), (call(I=40), SHAPE),
             (call(H=256 + 32, dg=G.DT_Q4_K), SHAPE), (call(H=0), SHAPE), (call(wb=c["total"] - 1), SHAPE), (call(wb=0), SHAPE),
             (call(x=c["xn"].ptr + 4), ALIGN), (call(g=c["dev"]["g"].ptr + 1), ALIGN)]
    ops.synchronize()
    for n, (got, want) in enumerate(calls):
        assert got == want, (n, got, want)
    assert y.untouched() and np.all(ws.numpy(np.uint32) == bits(np.full(1, POISON_F))[0])
    assert call() == 0          # ... and the same buffers take a good call afterwards
    assert np.abs(y.read().astype(np.float64) - c["y64"]).max() <= tol_for(c["y64"], I)
    ws.free(); y.dev.free()
