"""The grouped expert GEMM of the prompt pass on the GPU (csrc/moe_gemm.hip) through the C ABI: ntk_moe_gemm_gate_up and ntk_moe_gemm_down against the oracle's
GEMVs per pair, at the project's GEMV bars (tests/moe_ref.tol_for: 4e-6 sqrt(in) max(1, |ref|max)) -- F32 arithmetic in another summation order, so no
new tolerance.

Work lists.  E = 4, K = 2 with test_moe_gpu.hand_ids (expert 2 nobody, expert 1 every row, 0 and 3 by turns) at 1 / 2 / 15 / 16 / 17 / 33 rows: expert 1
then holds a lone pair, a full tile, a full tile plus one, two full tiles plus one.  One E = 8, K = 3 list in which expert 2 holds exactly 16 pairs, expert 3
none and expert 4 one.  Shapes (hidden, I_e): (64, 32) Q8_0 (fewer columns than a 256-column step), (256, 256) and (2048, 768) for Q8_0 / Q4_K / Q6_K and
Q4_K gate with Q6_K up and down, (32, 4352) Q8_0 (a down row of 17 steps: the wave's accumulators carry it).

Checked: every act row and every y row (from the oracle's act, and chained) at the bars; the same bits on a second launch; each of the 33 rows alone, the
rows reversed, a row behind 16 foreign rows (another tile and column): the bits of the 33-row launch; y in place over resid; the combine on a hand-filled
part against the GEMV form's; a NaN token row changes its own K pairs only; guard floats behind act / part / y, xn and resid unchanged; a foreign work list
(offsets and pair indices out of range) runs and writes nothing for the bad entries; every refusal over poisoned outputs.  The largest deviations are
printed per case (profiles/moe_gemm.txt records them).

Run on the MI355X box:  python -m pytest tests/test_moe_gemm_gpu.py -m gpu -x -q -s"""
import numpy as np
import pytest

from moe_ref import tol_for, work_list
from ntransformer_amd import _lib, gguf as G, ops
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O
from test_moe_gpu import POISON_F, TYPES, Out, bits, hand_ids

pytestmark = pytest.mark.gpu
ROWS = (1, 2, 15, 16, 17, 33)
T_ALL = 33
CASES = [("Q8_0", "Q8_0", "Q8_0", 64, 32), ("Q8_0", "Q8_0", "Q8_0", 32, 4352)]
for _g, _u, _d in (("Q8_0", "Q8_0", "Q8_0"), ("Q4_K", "Q4_K", "Q4_K"), ("Q6_K", "Q6_K", "Q6_K"), ("Q4_K", "Q6_K", "Q6_K")):
    CASES += [(_g, _u, _d, 256, 256), (_g, _u, _d, 2048, 768)]


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def ids_e8k3(T=16):
    """E = 8, K = 3: expert 2 every row (exactly 16 pairs), expert 3 nobody, expert 4 row 0 only, the rest over 0 / 1 / 5 / 6 / 7"""
    others = (0, 1, 5, 6, 7)
    rows = []
    for t in range(T):
        a, b = others[t % 5], others[(t + 2) % 5]
        row = [2, a, b] if t % 2 else [a, 2, b]
        if t == 0:
            row[2] = 4
        rows.append(row)
    ids = np.asarray(rows, np.int32)
    assert (ids == 2).sum() == 16 and (ids == 3).sum() == 0 and (ids == 4).sum() == 1 and all(len(set(r)) == 3 for r in rows)
    return ids


_cases = {}


def ffn_case(g, u, d, hidden, inter, E=4, K=2, T=T_ALL, ids=None):
    """expert tensors, rows, and the oracle's act [T K][inter] and y [T][hidden], once per session and read only"""
    key = (g, u, d, hidden, inter, E, K, T)
    if key not in _cases:
        r = np.random.Generator(np.random.Philox(key=[20261121, ((hidden * 10000 + inter) * 100 + E) * 1000000 + TYPES[g] * 10000 + TYPES[u] * 100 + TYPES[d]]))
        tt = {"g": g, "u": u, "d": d}
        W = {n: np.frombuffer(G.synth_tensor(r, TYPES[tt[n]], E * rows, cols), np.uint8) for n, rows, cols in (("g", inter, hidden), ("u", inter, hidden), ("d", hidden, inter))}
        xn = r.standard_normal((T, hidden)).astype(np.float32)
        resid = r.standard_normal((T, hidden)).astype(np.float32)
        w = r.uniform(0.1, 1.0, (T, K)).astype(np.float32)
        w = (w / w.sum(1, keepdims=True)).astype(np.float32)
        ids = hand_ids(T) if ids is None else ids
        dt = {n: G.GGML_TO_DT[TYPES[tt[n]]] for n in tt}

        def block(n, e, rows, cols):
            nb = rows * G.row_bytes(TYPES[tt[n]], cols)
            return W[n][e * nb:(e + 1) * nb]
        act = np.zeros((T * K, inter), np.float32)
        y = np.zeros((T, hidden), np.float32)
        for t in range(T):
            s = np.zeros(hidden, np.float32)
            for k in range(K):
                e = int(ids[t, k])
                a = O.silu_mul(O.gemv(block("g", e, inter, hidden), xn[t], inter, hidden, dt["g"]), O.gemv(block("u", e, inter, hidden), xn[t], inter, hidden, dt["u"]))
                act[t * K + k] = a
                s = (s + w[t, k] * O.gemv(block("d", e, hidden, inter), a, hidden, inter, dt["d"])).astype(np.float32)
            y[t] = resid[t] + s
        for a in (xn, resid, w, ids, act, y):
            a.setflags(write=False)
        _cases[key] = dict(W=W, dt=dt, xn=xn, resid=resid, w=w, ids=ids, act=act, y=y, E=E, K=K, hidden=hidden, inter=inter, dev={n: DB.from_numpy(W[n]) for n in W})
    return _cases[key]


def run_ffn(c, rows, alias=False, act_in=None, xn=None, gemv=False, keep_part=False):
    """the GEMM pair (gemv: the GEMV pair) on the given rows of the case: (act [n K][inter], y [n][hidden][, part]); act_in: the down launch reads these rows.
    Guards behind act / part / y are checked by Out.read; xn and resid must come back unchanged."""
    n, E, K, hidden, inter = len(rows), c["E"], c["K"], c["hidden"], c["inter"]
    ids, w = c["ids"][rows], c["w"][rows]
    x_in = np.ascontiguousarray((c["xn"] if xn is None else xn)[rows])
    offsets, pairs = work_list(ids, E)
    dx, dres = DB.from_numpy(x_in), DB.from_numpy(c["resid"][rows])
    dids, dw, doff, dpairs = DB.from_numpy(np.ascontiguousarray(ids)), DB.from_numpy(np.ascontiguousarray(w)), DB.from_numpy(offsets), DB.from_numpy(pairs)
    act = Out(n * K * inter, np.float32)
    if gemv:
        ops.moe_gate_up(act.ptr, dx, c["dev"]["g"], c["dt"]["g"], c["dev"]["u"], c["dt"]["u"], doff, dpairs, n, hidden, inter, E, K)
    else:
        need = ops.moe_gemm_scratch_bytes(n, E, K, inter, hidden)
        scratch = DB(need) if need else None
        ops.moe_gemm_gate_up(act.ptr, dx, c["dev"]["g"], c["dt"]["g"], c["dev"]["u"], c["dt"]["u"], doff, dpairs, n, hidden, inter, E, K, scratch, need)
        ops.synchronize()
        if scratch:
            scratch.free()
    got_act = act.read().reshape(n * K, inter)
    dact = DB.from_numpy(np.ascontiguousarray(got_act if act_in is None else act_in))
    part = Out(n * K * hidden, np.float32)
    y = Out(n * hidden, np.float32)
    if alias:
        y.dev.upload(np.ascontiguousarray(c["resid"][rows]))
    down = ops.moe_down if gemv else ops.moe_gemm_down
    down(y.ptr, y.ptr if alias else dres, dact, c["dev"]["d"], c["dt"]["d"], dids, dw, doff, dpairs, part.ptr, n, hidden, inter, E, K)
    got_y = y.read().reshape(n, hidden)
    got_part = part.read().reshape(n * K, hidden)
    assert np.array_equal(bits(dres.numpy(np.float32, n * hidden)), bits(c["resid"][rows].reshape(-1))), "resid changed"
    assert np.array_equal(bits(dx.numpy(np.float32, n * hidden)), bits(x_in.reshape(-1))), "xn changed"
    for b in (dx, dres, dids, dw, doff, dpairs, dact):
        b.free()
    return (got_act, got_y, got_part) if keep_part else (got_act, got_y)


def check_against_oracle(c, rows, tag):
    """act, y from the oracle's act, y in place, the chained y, a second launch; returns (act, y, worst act ratio, worst y ratio) of the chained run"""
    K, hidden, inter = c["K"], c["hidden"], c["inter"]
    act, y = run_ffn(c, rows)
    pairs_of = [t * K + k for t in rows for k in range(K)]
    worst_a = worst_y = 0.0
    for i, p in enumerate(pairs_of):
        err = float(np.abs(act[i] - c["act"][p]).max())
        worst_a = max(worst_a, err / tol_for(c["act"][p], hidden))
        assert err <= tol_for(c["act"][p], hidden), (tag, "act", p, err, tol_for(c["act"][p], hidden))
    _, y_o = run_ffn(c, rows, act_in=c["act"][pairs_of])          # the down launch on the ORACLE's act rows: its own error alone
    _, y_alias = run_ffn(c, rows, alias=True, act_in=c["act"][pairs_of])
    for i, t in enumerate(rows):
        for name, yy in (("y", y_o), ("chained y", y)):
            err = float(np.abs(yy[i] - c["y"][t]).max())
            worst_y = max(worst_y, err / tol_for(c["y"][t], inter))
            assert err <= tol_for(c["y"][t], inter), (tag, name, t, err, tol_for(c["y"][t], inter))
    assert np.array_equal(bits(y_alias), bits(y_o)), (tag, "in place")
    act2, y2 = run_ffn(c, rows)
    assert np.array_equal(bits(act2), bits(act)) and np.array_equal(bits(y2), bits(y)), (tag, "second launch")
    return act, y, worst_a, worst_y


@pytest.mark.parametrize("g,u,d,hidden,inter", CASES)
def test_gemm_pair_against_the_oracle_and_its_own_bits(g, u, d, hidden, inter):
    c = ffn_case(g, u, d, hidden, inter)
    K = c["K"]
    full, wa, wy = None, 0.0, 0.0
    for T in ROWS:
        act, y, a, b = check_against_oracle(c, list(range(T)), (g, u, d, hidden, inter, T))
        wa, wy = max(wa, a), max(wy, b)
        if T == T_ALL:
            full = (act, y)
    print("moe_gemm %s/%s/%s (%d, %d): largest act error %.3f of its bar, largest y error %.3f of its bar" % (g, u, d, hidden, inter, wa, wy))
    fa = full[0].reshape(T_ALL, K, inter)
    for t in range(T_ALL):          # each row alone: the bits it has among the 33
        a1, y1 = run_ffn(c, [t])
        assert np.array_equal(bits(a1), bits(fa[t])), t
        assert np.array_equal(bits(y1[0]), bits(full[1][t])), t
    ar, yr = run_ffn(c, list(range(T_ALL - 1, -1, -1)))          # reversed rows give reversed results
    assert np.array_equal(bits(yr[::-1]), bits(full[1]))
    assert np.array_equal(bits(ar.reshape(T_ALL, K, inter)[::-1]), bits(fa))
    for t in (16, 21, 32):          # behind 16 foreign rows: another tile, another column
        rows = list(range(16)) + [t]
        a2, y2 = run_ffn(c, rows)
        assert np.array_equal(bits(a2.reshape(17, K, inter)[16]), bits(fa[t])), t
        assert np.array_equal(bits(y2[16]), bits(full[1][t])), t
        assert np.array_equal(bits(y2[:16]), bits(full[1][:16]))


def test_a_list_with_a_full_tile_an_empty_neighbour_and_a_lone_pair():
    T = 16
    c = ffn_case("Q8_0", "Q8_0", "Q8_0", 256, 256, E=8, K=3, T=T, ids=ids_e8k3(T))
    off, _ = work_list(c["ids"], 8)
    assert list(np.diff(off)[2:5]) == [16, 0, 1]
    _, _, wa, wy = check_against_oracle(c, list(range(T)), "e8k3")
    print("moe_gemm E 8 / K 3 list: largest act error %.3f of its bar, largest y error %.3f of its bar" % (wa, wy))


def test_the_combine_is_the_gemv_forms_on_a_hand_filled_part():
    """an EMPTY work list (no launch writes part) under real ids and weights: both forms then sum the part we filled"""
    c = ffn_case("Q8_0", "Q8_0", "Q8_0", 256, 256)
    T, E, K, hidden, inter = 17, c["E"], c["K"], 256, 256
    r = np.random.Generator(np.random.Philox(key=[20261121, 5]))
    part_np = r.standard_normal((T * K, hidden)).astype(np.float32)
    ids = np.ascontiguousarray(c["ids"][:T]).copy()
    ids[3, 1] = -1          # (an id out of range: its term is skipped by both)
    bufs = [DB.from_numpy(a) for a in (ids, np.ascontiguousarray(c["w"][:T]), np.zeros(E + 1, np.int32), np.zeros(T * K, np.int32), np.ascontiguousarray(c["act"][:T * K]),
                                       np.ascontiguousarray(c["resid"][:T]))]
    dids, dw, doff, dpairs, dact, dres = bufs
    got = []
    for fn in (ops.moe_down, ops.moe_gemm_down):
        part, y = DB.from_numpy(part_np), Out(T * hidden, np.float32)
        fn(y.ptr, dres, dact, c["dev"]["d"], c["dt"]["d"], dids, dw, doff, dpairs, part, T, hidden, inter, E, K)
        got.append(y.read())
        assert np.array_equal(bits(part.numpy(np.float32, T * K * hidden)), bits(part_np.reshape(-1)))
        part.free()
    assert np.array_equal(bits(got[0]), bits(got[1]))
    want = c["resid"][:T].astype(np.float64).copy()
    for t in range(T):
        for k in range(K):
            if ids[t, k] >= 0:
                want[t] += float(c["w"][t, k]) * part_np[t * K + k].astype(np.float64)
    assert np.abs(got[1].reshape(T, hidden) - want).max() <= 1e-5
    for b in bufs:
        b.free()


def test_a_nan_token_row_stays_in_its_own_pairs():
    c = ffn_case("Q4_K", "Q6_K", "Q6_K", 256, 256)
    T, K = 17, c["K"]
    rows = list(range(T))
    act, y = run_ffn(c, rows)
    xn = c["xn"].copy()
    xn[5] = np.nan
    act_n, y_n = run_ffn(c, rows, xn=xn)
    mine = [5 * K + k for k in range(K)]
    rest = [p for p in range(T * K) if p not in mine]
    assert np.isnan(act_n[mine]).all() and np.isnan(y_n[5]).all()
    assert np.array_equal(bits(act_n[rest]), bits(act[rest]))
    assert np.array_equal(bits(np.delete(y_n, 5, 0)), bits(np.delete(y, 5, 0)))


def test_a_foreign_work_list_stays_inside_the_buffers():
    """offsets below 0 and beyond the list, pair indices outside [0, T K), in an oversized pairs buffer: NTK_OK, and nothing is written for the bad entries"""
    c = ffn_case("Q8_0", "Q8_0", "Q8_0", 256, 256)
    T, E, K, hidden, inter = 4, c["E"], c["K"], 256, 256
    n_pairs = T * K
    offsets = np.asarray([-5, 3, 3, 100, 200], np.int32)          # expert 0: [0, 3), expert 1: nothing, expert 2: [3, 8) after the clamp, expert 3: nothing
    pairs = np.full(64, 7, np.int32)
    pairs[:n_pairs] = [0, -1, 9, 3, 1000000, 5, 8, 7]
    good = {0: 0, 3: 2, 5: 2, 7: 2}          # pair -> the expert whose range names it
    xn, resid, w = c["xn"][:T], c["resid"][:T], c["w"][:T]
    tt = {"g": "Q8_0", "u": "Q8_0", "d": "Q8_0"}

    def block(n, e, rows, cols):
        nb = rows * G.row_bytes(TYPES[tt[n]], cols)
        return c["W"][n][e * nb:(e + 1) * nb]
    act_ref = np.zeros((n_pairs, inter), np.float32)
    ids = np.full((T, K), -1, np.int32)
    y_ref = resid.copy()
    for p, e in good.items():
        t = p // K
        ids[t, p % K] = e
        act_ref[p] = O.silu_mul(O.gemv(block("g", e, inter, hidden), xn[t], inter, hidden, c["dt"]["g"]), O.gemv(block("u", e, inter, hidden), xn[t], inter, hidden, c["dt"]["u"]))
    for t in range(T):
        s = np.zeros(hidden, np.float32)
        for k in range(K):
            if ids[t, k] >= 0:
                s = (s + w[t, k] * O.gemv(block("d", int(ids[t, k]), hidden, inter), act_ref[t * K + k], hidden, inter, c["dt"]["d"])).astype(np.float32)
        y_ref[t] = resid[t] + s
    bufs = [DB.from_numpy(np.ascontiguousarray(a)) for a in (xn, resid, w, ids, offsets, pairs, act_ref)]
    dx, dres, dw, dids, doff, dpairs, dact = bufs
    L = _lib.lib()
    act, part, y = Out(n_pairs * inter, np.float32), Out(n_pairs * hidden, np.float32), Out(T * hidden, np.float32)
    assert L.ntk_moe_gemm_gate_up(act.ptr, dx.ptr, c["dev"]["g"].ptr, c["dt"]["g"], c["dev"]["u"].ptr, c["dt"]["u"], doff.ptr, dpairs.ptr, None, 0, T, hidden, inter, E, K, None) == 0
    assert L.ntk_moe_gemm_down(y.ptr, dres.ptr, dact.ptr, c["dev"]["d"].ptr, c["dt"]["d"], dids.ptr, dw.ptr, doff.ptr, dpairs.ptr, part.ptr, T, hidden, inter, E, K, None) == 0
    ops.synchronize()
    got_act, got_part, got_y = act.read().reshape(n_pairs, inter), part.read().reshape(n_pairs, hidden), y.read().reshape(T, hidden)
    for p in range(n_pairs):
        if p in good:
            assert np.abs(got_act[p] - act_ref[p]).max() <= tol_for(act_ref[p], hidden), p
        else:
            assert np.array_equal(bits(got_act[p]), bits(np.full(inter, POISON_F, np.float32))), p
            assert np.array_equal(bits(got_part[p]), bits(np.full(hidden, POISON_F, np.float32))), p
    for t in range(T):
        assert np.abs(got_y[t] - y_ref[t]).max() <= tol_for(y_ref[t], inter), t
    for b in bufs:
        b.free()


def test_refusals_leave_the_outputs_untouched():
    hidden, inter, T = 64, 32, 2
    c = ffn_case("Q8_0", "Q8_0", "Q8_0", hidden, inter)
    E, K = c["E"], c["K"]
    L = _lib.lib()
    ids, w = np.ascontiguousarray(c["ids"][:T]), np.ascontiguousarray(c["w"][:T])
    offsets, pairs = work_list(ids, E)
    dx, dres = DB.from_numpy(c["xn"][:T]), DB.from_numpy(c["resid"][:T])
    dids, dw, doff, dpairs = DB.from_numpy(ids), DB.from_numpy(w), DB.from_numpy(offsets), DB.from_numpy(pairs)
    dact_in = DB.from_numpy(c["act"][:T * K])
    act, y, part = Out(1024 * 16 * inter, np.float32), Out(T * hidden, np.float32), Out(1024 * 16 * hidden, np.float32)
    Wg, Wu, Wd = c["dev"]["g"].ptr, c["dev"]["u"].ptr, c["dev"]["d"].ptr
    q8, f16, q40, q5k = G.DT_Q8_0, G.DT_F16, G.DT_Q4_0, G.DT_Q5_K
    need = int(L.ntk_moe_gemm_scratch_bytes(T, E, K, inter, hidden))
    scratch = DB(max(need, 16))

    def gate_up(a=act.ptr, x=dx.ptr, g=Wg, dg=q8, u=Wu, du=q8, off=doff.ptr, pr=dpairs.ptr, sc=scratch.ptr, sb=need, T=T, H=hidden, I=inter, E=E, K=K):
        return L.ntk_moe_gemm_gate_up(a, x, g, dg, u, du, off, pr, sc, sb, T, H, I, E, K, None)

    def down(yy=y.ptr, r=dres.ptr, a=dact_in.ptr, d=Wd, dd=q8, i=dids.ptr, ww=dw.ptr, off=doff.ptr, pr=dpairs.ptr, pt=part.ptr, T=T, H=hidden, I=inter, E=E, K=K):
        return L.ntk_moe_gemm_down(yy, r, a, d, dd, i, ww, off, pr, pt, T, H, I, E, K, None)
    NULL, SHAPE, DTYPE, ALIGN = -5, -2, -1, -4
    calls = [
        (gate_up(a=None), NULL), (gate_up(x=None), NULL), (gate_up(g=None), NULL), (gate_up(u=None), NULL), (gate_up(off=None), NULL), (gate_up(pr=None), NULL),
        (gate_up(dg=f16), DTYPE), (gate_up(du=q40), DTYPE), (gate_up(dg=q5k), DTYPE), (gate_up(du=f16), DTYPE),
        (gate_up(T=0), SHAPE), (gate_up(T=1025), SHAPE), (gate_up(E=257), SHAPE), (gate_up(K=17, E=32), SHAPE), (gate_up(K=5), SHAPE), (gate_up(K=0), SHAPE),
        (gate_up(H=48), SHAPE), (gate_up(H=256 + 32, dg=G.DT_Q4_K, du=G.DT_Q4_K), SHAPE), (gate_up(I=0), SHAPE),
        (gate_up(a=act.ptr + 4), ALIGN), (gate_up(x=dx.ptr + 4), ALIGN), (gate_up(g=Wg + 1), ALIGN),
        (down(yy=None), NULL), (down(r=None), NULL), (down(a=None), NULL), (down(d=None), NULL), (down(i=None), NULL), (down(ww=None), NULL),
        (down(off=None), NULL), (down(pr=None), NULL), (down(pt=None), NULL),
        (down(dd=f16), DTYPE), (down(dd=q40), DTYPE), (down(dd=q5k), DTYPE),
        (down(T=0), SHAPE), (down(T=1025), SHAPE), (down(E=257), SHAPE), (down(K=17, E=32), SHAPE), (down(K=5), SHAPE),
        (down(I=40), SHAPE), (down(I=256 + 32, dd=G.DT_Q6_K), SHAPE), (down(a=dact_in.ptr + 4), ALIGN), (down(d=Wd + 1), ALIGN),
    ]
    if need > 0:          # (today the size is 0 for every shape: nothing can be below it)
        calls += [(gate_up(sb=need - 1), SHAPE), (gate_up(sc=None), NULL)]
    else:
        assert L.ntk_moe_gemm_scratch_bytes(0, E, K, inter, hidden) == 0 and L.ntk_moe_gemm_scratch_bytes(T, 257, K, inter, hidden) == 0
    # the GEMV form answers the same faults with the same codes
    for kw, want in ((dict(dg=f16), DTYPE), (dict(T=1025), SHAPE), (dict(K=5), SHAPE), (dict(H=48), SHAPE), (dict(x=dx.ptr + 4), ALIGN), (dict(a=None), NULL)):
        p = dict(a=act.ptr, x=dx.ptr, g=Wg, dg=q8, u=Wu, du=q8, off=doff.ptr, pr=dpairs.ptr, T=T, H=hidden, I=inter, E=E, K=K)
        p.update(kw)
        assert L.ntk_moe_gate_up(p["a"], p["x"], p["g"], p["dg"], p["u"], p["du"], p["off"], p["pr"], p["T"], p["H"], p["I"], p["E"], p["K"], None) == want
    ops.synchronize()
    for n, (got, want) in enumerate(calls):
        assert got == want, (n, got, want)
    for o in (act, y, part):
        assert o.untouched()
    assert gate_up() == 0 and down() == 0          # ... and the same buffers take a good call afterwards
    ops.synchronize()
    assert np.abs(y.read().reshape(T, hidden) - c["y"][:T]).max() <= tol_for(c["y"][:T], inter)
    for b in (dx, dres, dids, dw, doff, dpairs, dact_in, scratch):
        b.free()
