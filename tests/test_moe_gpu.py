"""The three launches of the routed expert FFN on the GPU (csrc/moe.hip) through the C ABI: ntk_moe_route, ntk_moe_gate_up, ntk_moe_down.

ntk_moe_route at T = 1 / 2 / 17, E = 4 / 8 / 128 / 256, K = 1 / 2 / 8 / 16 on logits that are EXACT by construction: row t of xn is one-hot at column t
plus a 2 in the last column, router entries are small integers, so every logit is an integer whatever the summation order, all logits of a row differ and
the gaps are >= 1.  ids and the work list must equal numpy's (a stable argsort) exactly, w the float64 softmax over the selected logits within 1e-6 (a
few F32 roundings on values <= 1), the optional logits the integers.  Duplicated router rows give ties: the lower index must win.  Random xn at hidden
64 / 2048: logits within tol_for.  The same bits on three launches; guard words behind every output keep their bits.

ntk_moe_gate_up / ntk_moe_down for Q8_0 at (hidden, I_e) = (64, 32) and (2048, 768), for Q4_K / Q6_K and the mixed pairs (Q4_K gate with Q6_K up, a Q6_K
down: 630-byte rows at I_e = 768) at (256, 256) and (2048, 768), E = 4, K = 2, hand-written ids at T = 1 / 2 / 17: expert 2 nobody chose, expert 1 chosen by
all 17 rows, the last expert chosen by some.  Every act row against O.silu_mul of the oracle's two GEMVs and every y row against the oracle's weighted
sum, both at tol_for (4e-6 sqrt(in) max(1, |ref|max): the project's GEMV bar); y aliasing resid and not; a pair's bits with 16 companions equal its bits
alone; the same bits on repeat; reversed rows give reversed results; guards behind T K rows untouched; every refusal over poisoned outputs.

Run on the MI355X box:  python -m pytest tests/test_moe_gpu.py -m gpu -x -q"""
import numpy as np
import pytest

from moe_ref import select_experts, tol_for, work_list
from ntransformer_amd import _lib, gguf as G, ops
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O

pytestmark = pytest.mark.gpu
GUARD = 16
POISON_F, POISON_I = np.float32(-7.25e8), np.int32(-1234567)
ROWS = (1, 2, 17)


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Out:
    """n values on the device with GUARD poisoned words behind them"""

    def __init__(self, n, dtype):
        self.n, self.dtype = n, dtype
        self.poison = POISON_F if dtype == np.float32 else POISON_I
        self.dev = DB.from_numpy(np.full(n + GUARD, self.poison, dtype))
        self.ptr = self.dev.ptr

    def read(self):
        got = self.dev.numpy(self.dtype, self.n + GUARD)
        assert np.array_equal(bits(got[self.n:]), bits(np.full(GUARD, self.poison, self.dtype))), "wrote behind the output"
        return got[:self.n].copy()

    def untouched(self):
        got = self.dev.numpy(self.dtype, self.n + GUARD)
        return np.array_equal(bits(got), bits(np.full(self.n + GUARD, self.poison, self.dtype)))


# ------------------------------------------------------------------------------------------------ routing
def route(xn, router, T, hidden, E, K, with_logits=True):
    dx, dr = DB.from_numpy(xn.astype(np.float32)), DB.from_numpy(router.astype(np.float32))
    ids, w, off, pairs = Out(T * K, np.int32), Out(T * K, np.float32), Out(E + 1, np.int32), Out(T * K, np.int32)
    lg = Out(T * E, np.float32) if with_logits else None
    ops.moe_route(dx, dr, T, hidden, E, K, ids.ptr, w.ptr, off.ptr, pairs.ptr, lg.ptr if lg else None)
    ops.synchronize()
    res = dict(ids=ids.read().reshape(T, K), w=w.read().reshape(T, K), offsets=off.read(), pairs=pairs.read(), logits=lg.read().reshape(T, E) if lg else None)
    dx.free(); dr.free()
    return res


def exact_case(T, E, seed, ties=False):
    """xn [T][32] and an integer router [E][32] whose logits are distinct integers per row (ties: expert pairs (1, E - 2) and (0, E - 1) share a row)"""
    r = np.random.Generator(np.random.Philox(key=[20261101, seed]))
    hidden = 32
    xn = np.zeros((T, hidden), np.float32)
    router = r.integers(-3, 4, (E, hidden)).astype(np.float32)
    for t in range(T):
        xn[t, t] = 1.0
        xn[t, hidden - 1] = 2.0
        router[:, t] = 3.0 * (r.permutation(E) - E // 2)
    router[:, hidden - 1] = r.integers(0, 2, E)
    if ties and E >= 4:
        router[E - 2] = router[1]
        router[E - 1] = router[0]
        router[1, 0] = router[E - 2, 0] = 3.0 * E          # row 0: the twins 1 and E - 2 lead, so K >= 2 selects both
    return xn, router, hidden


def check_route(res, logits_want, T, E, K):
    for t in range(T):
        want = select_experts(logits_want[t], K)
        assert np.array_equal(res["ids"][t], want), (t, res["ids"][t], want)
        sel = logits_want[t][want].astype(np.float64)
        p = np.exp(sel - sel.max())
        assert np.abs(res["w"][t].astype(np.float64) - p / p.sum()).max() <= 1e-6
    flat = res["ids"].reshape(-1)
    assert np.array_equal(res["pairs"], np.argsort(flat, kind="stable").astype(np.int32))
    assert np.array_equal(res["offsets"], np.concatenate([[0], np.cumsum(np.bincount(flat, minlength=E))]).astype(np.int32))
    off2, pairs2 = work_list(res["ids"], E)
    assert np.array_equal(off2, res["offsets"]) and np.array_equal(pairs2, res["pairs"])


@pytest.mark.parametrize("E,K", [(4, 1), (4, 2), (8, 2), (8, 8), (128, 8), (128, 16), (256, 1), (256, 16)])
@pytest.mark.parametrize("T", ROWS)
def test_route_on_exact_integer_logits(T, E, K):
    xn, router, hidden = exact_case(T, E, 100 * E + K)
    want = (xn.astype(np.float64) @ router.astype(np.float64).T).astype(np.float32)
    assert all(np.diff(np.sort(want[t])).min() >= 1.0 for t in range(T))
    res = route(xn, router, T, hidden, E, K)
    assert np.array_equal(res["logits"], want)
    check_route(res, want, T, E, K)
    again = [route(xn, router, T, hidden, E, K, with_logits=False) for _ in range(2)]          # (and without the optional logits)
    for a in again:
        for key in ("ids", "offsets", "pairs"):
            assert np.array_equal(a[key], res[key])
        assert np.array_equal(bits(a["w"]), bits(res["w"]))


@pytest.mark.parametrize("E,K", [(4, 2), (8, 2), (128, 8), (256, 16)])
def test_route_ties_go_to_the_lower_expert(E, K):
    T = 17
    xn, router, hidden = exact_case(T, E, 7000 + E, ties=True)
    want = (xn.astype(np.float64) @ router.astype(np.float64).T).astype(np.float32)
    assert np.array_equal(want[:, 1], want[:, E - 2]) and np.array_equal(want[:, 0], want[:, E - 1])
    res = route(xn, router, T, hidden, E, K)
    assert np.array_equal(res["logits"], want)
    check_route(res, want, T, E, K)
    seen = 0
    for t in range(T):          # wherever both twins are selected the lower index stands first
        ids = list(res["ids"][t])
        for lo, hi in ((1, E - 2), (0, E - 1)):
            if lo in ids and hi in ids:
                assert ids.index(lo) + 1 == ids.index(hi)
                seen += 1
            assert not (hi in ids and lo not in ids)
    assert seen > 0


@pytest.mark.parametrize("hidden", [64, 2048])
def test_route_logits_on_random_rows(hidden):
    T, E, K = 17, 128, 8
    r = np.random.Generator(np.random.Philox(key=[20261101, hidden]))
    xn = r.standard_normal((T, hidden)).astype(np.float32)
    router = (r.standard_normal((E, hidden)) / np.sqrt(hidden)).astype(np.float32)
    res = route(xn, router, T, hidden, E, K)
    for t in range(T):
        want = O.gemv(router, xn[t], E, hidden, G.DT_F32)
        err = float(np.abs(res["logits"][t] - want).max())
        assert err <= tol_for(want, hidden), (t, err)
        assert np.array_equal(res["ids"][t], select_experts(res["logits"][t], K))          # the selection of the launch's own logits
    check_route(res, res["logits"], T, E, K)


# ------------------------------------------------------------------------------------------------ gate | up and down
E4, K2 = 4, 2
TYPES = {"Q8_0": G.GGML_Q8_0, "Q4_K": G.GGML_Q4_K, "Q6_K": G.GGML_Q6_K}
CASES = [("Q8_0", "Q8_0", "Q8_0", 64, 32), ("Q8_0", "Q8_0", "Q8_0", 2048, 768)]
for _g, _u, _d in (("Q4_K", "Q4_K", "Q4_K"), ("Q6_K", "Q6_K", "Q6_K"), ("Q4_K", "Q6_K", "Q6_K")):
    CASES += [(_g, _u, _d, 256, 256), (_g, _u, _d, 2048, 768)]


def hand_ids(T):
    """expert 2: nobody; expert 1: every row; the last expert (3) and expert 0 by turns, in either slot"""
    rows = []
    for t in range(T):
        other = 3 if t % 2 == 0 else 0
        rows.append((other, 1) if t % 3 == 0 else (1, other))
    return np.asarray(rows, np.int32)


_models = {}


def ffn_case(g, u, d, hidden, inter):
    """expert tensors, rows, and the oracle's results for T = 17, once per session"""
    key = (g, u, d, hidden, inter)
    if key not in _models:
        r = np.random.Generator(np.random.Philox(key=[20261101, (hidden * 1000 + inter) * 1000000 + TYPES[g] * 10000 + TYPES[u] * 100 + TYPES[d]]))
        W = {n: np.frombuffer(G.synth_tensor(r, TYPES[t], E4 * rows, cols), np.uint8)
             for n, t, rows, cols in (("g", g, inter, hidden), ("u", u, inter, hidden), ("d", d, hidden, inter))}
        T = 17
        xn = r.standard_normal((T, hidden)).astype(np.float32)
        resid = r.standard_normal((T, hidden)).astype(np.float32)
        w = r.uniform(0.1, 1.0, (T, K2)).astype(np.float32)
        w = (w / w.sum(1, keepdims=True)).astype(np.float32)
        ids = hand_ids(T)
        dt = {n: G.GGML_TO_DT[TYPES[t]] for n, t in (("g", g), ("u", u), ("d", d))}

        def block(n, e, rows, cols):
            nb = rows * G.row_bytes(TYPES[{"g": g, "u": u, "d": d}[n]], cols)
            return W[n][e * nb:(e + 1) * nb]
        act = np.zeros((T * K2, inter), np.float32)
        y = np.zeros((T, hidden), np.float32)
        for t in range(T):
            s = np.zeros(hidden, np.float32)
            for k in range(K2):
                e = int(ids[t, k])
                a = O.silu_mul(O.gemv(block("g", e, inter, hidden), xn[t], inter, hidden, dt["g"]), O.gemv(block("u", e, inter, hidden), xn[t], inter, hidden, dt["u"]))
                act[t * K2 + k] = a
                s = (s + w[t, k] * O.gemv(block("d", e, hidden, inter), a, hidden, inter, dt["d"])).astype(np.float32)
            y[t] = resid[t] + s
        _models[key] = dict(W=W, dt=dt, xn=xn, resid=resid, w=w, ids=ids, act=act, y=y, dev={n: DB.from_numpy(W[n]) for n in W})
    return _models[key]


def run_ffn(c, hidden, inter, rows, alias=False, act_in=None):
    """the two launches on the given rows of the case: (act [n K][inter], y [n][hidden]); act_in: the down launch reads these rows instead of the launch's own"""
    n = len(rows)
    ids, w = c["ids"][rows], c["w"][rows]
    offsets, pairs = work_list(ids, E4)
    dx, dres = DB.from_numpy(c["xn"][rows]), DB.from_numpy(c["resid"][rows])
    dids, dw, doff, dpairs = DB.from_numpy(ids), DB.from_numpy(w), DB.from_numpy(offsets), DB.from_numpy(pairs)
    act = Out(n * K2 * inter, np.float32)
    ops.moe_gate_up(act.ptr, dx, c["dev"]["g"], c["dt"]["g"], c["dev"]["u"], c["dt"]["u"], doff, dpairs, n, hidden, inter, E4, K2)
    got_act = act.read().reshape(n * K2, inter)
    dact = DB.from_numpy(got_act if act_in is None else act_in)
    part = DB(n * K2 * hidden * 4)
    if alias:
        y = Out(n * hidden, np.float32)
        y.dev.upload(c["resid"][rows])
        ops.moe_down(y.ptr, y.ptr, dact, c["dev"]["d"], c["dt"]["d"], dids, dw, doff, dpairs, part, n, hidden, inter, E4, K2)
    else:
        y = Out(n * hidden, np.float32)
        ops.moe_down(y.ptr, dres, dact, c["dev"]["d"], c["dt"]["d"], dids, dw, doff, dpairs, part, n, hidden, inter, E4, K2)
    got_y = y.read().reshape(n, hidden)
    assert np.array_equal(bits(dres.numpy(np.float32, n * hidden)), bits(c["resid"][rows].reshape(-1)))
    for b in (dx, dres, dids, dw, doff, dpairs, dact, part):
        b.free()
    return got_act, got_y


@pytest.mark.parametrize("g,u,d,hidden,inter", CASES)
def test_gate_up_and_down_against_the_oracle(g, u, d, hidden, inter):
    c = ffn_case(g, u, d, hidden, inter)
    full = None
    for T in ROWS:
        rows = list(range(T))
        act, y = run_ffn(c, hidden, inter, rows)
        for p in range(T * K2):
            err = float(np.abs(act[p] - c["act"][p]).max())
            assert err <= tol_for(c["act"][p], hidden), ("act", T, p, err)
        # the down launch on the ORACLE's act rows: its own error alone
        _, y_o = run_ffn(c, hidden, inter, rows, act_in=c["act"][:T * K2])
        _, y_alias = run_ffn(c, hidden, inter, rows, alias=True, act_in=c["act"][:T * K2])
        for t in range(T):
            err = float(np.abs(y_o[t] - c["y"][t]).max())
            assert err <= tol_for(c["y"][t], inter), ("y", T, t, err)
        assert np.array_equal(bits(y_alias), bits(y_o))          # in place on the hidden state: the same bits
        for t in range(T):          # ... and the chain gate | up -> down on the launch's own act rows, at the same bar
            err = float(np.abs(y[t] - c["y"][t]).max())
            assert err <= tol_for(c["y"][t], inter), ("chained y", T, t, err)
        act2, y2 = run_ffn(c, hidden, inter, rows)                # the same bits on repeat
        assert np.array_equal(bits(act2), bits(act)) and np.array_equal(bits(y2), bits(y))
        if T == 17:
            full = (act, y)
    # a pair's bits with 16 companions equal its bits alone
    for t in range(17):
        a1, y1 = run_ffn(c, hidden, inter, [t])
        assert np.array_equal(bits(a1), bits(full[0][t * K2:(t + 1) * K2])), t
        assert np.array_equal(bits(y1[0]), bits(full[1][t])), t
    # reversed rows give reversed results
    ar, yr = run_ffn(c, hidden, inter, list(range(16, -1, -1)))
    assert np.array_equal(bits(yr[::-1]), bits(full[1]))
    assert np.array_equal(bits(ar.reshape(17, K2, inter)[::-1]), bits(full[0].reshape(17, K2, inter)))


def test_refusals_leave_the_outputs_untouched():
    hidden, inter, T = 64, 32, 2
    c = ffn_case("Q8_0", "Q8_0", "Q8_0", hidden, inter)
    L = _lib.lib()
    ids, w = c["ids"][:T], c["w"][:T]
    offsets, pairs = work_list(ids, E4)
    dx, dres = DB.from_numpy(c["xn"][:T]), DB.from_numpy(c["resid"][:T])
    dids, dw, doff, dpairs = DB.from_numpy(ids), DB.from_numpy(w), DB.from_numpy(offsets), DB.from_numpy(pairs)
    dact_in = DB.from_numpy(c["act"][:T * K2])
    part = DB(T * K2 * hidden * 4)
    router = DB.from_numpy(np.ones((E4, hidden), np.float32))
    act, y = Out(1024 * 16 * inter, np.float32), Out(T * hidden, np.float32)
    o_ids, o_w, o_off, o_pairs = Out(64, np.int32), Out(64, np.float32), Out(300, np.int32), Out(64, np.int32)
    Wg, Wu, Wd = c["dev"]["g"].ptr, c["dev"]["u"].ptr, c["dev"]["d"].ptr
    q8, f16, q40, q5k = G.DT_Q8_0, G.DT_F16, G.DT_Q4_0, G.DT_Q5_K

    def gate_up(a=act.ptr, x=dx.ptr, g=Wg, dg=q8, u=Wu, du=q8, off=doff.ptr, pr=dpairs.ptr, T=T, H=hidden, I=inter, E=E4, K=K2):
        return L.ntk_moe_gate_up(a, x, g, dg, u, du, off, pr, T, H, I, E, K, None)

    def down(yy=y.ptr, r=dres.ptr, a=dact_in.ptr, d=Wd, dd=q8, i=dids.ptr, ww=dw.ptr, off=doff.ptr, pr=dpairs.ptr, pt=part.ptr, T=T, H=hidden, I=inter, E=E4, K=K2):
        return L.ntk_moe_down(yy, r, a, d, dd, i, ww, off, pr, pt, T, H, I, E, K, None)

    def rt(x=dx.ptr, r=router.ptr, T=T, H=hidden, E=E4, K=K2, i=o_ids.ptr, ww=o_w.ptr, off=o_off.ptr, pr=o_pairs.ptr):
        return L.ntk_moe_route(x, r, T, H, E, K, i, ww, off, pr, None, None)
    NULL, SHAPE, DTYPE = -5, -2, -1
    calls = [
        (gate_up(a=None), NULL), (gate_up(x=None), NULL), (gate_up(g=None), NULL), (gate_up(u=None), NULL), (gate_up(off=None), NULL), (gate_up(pr=None), NULL),
        (gate_up(dg=f16), DTYPE), (gate_up(du=q40), DTYPE), (gate_up(dg=q5k), DTYPE), (gate_up(dg=G.DT_BF16), DTYPE),
        (gate_up(K=5), SHAPE), (gate_up(E=257), SHAPE), (gate_up(T=0), SHAPE), (gate_up(T=1025), SHAPE), (gate_up(K=0), SHAPE), (gate_up(K=17, E=32), SHAPE),
        (gate_up(H=48), SHAPE), (gate_up(H=256 + 32, dg=G.DT_Q4_K, du=G.DT_Q4_K), SHAPE), (gate_up(I=0), SHAPE),
        (down(yy=None), NULL), (down(r=None), NULL), (down(a=None), NULL), (down(d=None), NULL), (down(i=None), NULL), (down(ww=None), NULL),
        (down(off=None), NULL), (down(pr=None), NULL), (down(pt=None), NULL),
        (down(dd=f16), DTYPE), (down(dd=q5k), DTYPE), (down(K=5), SHAPE), (down(E=257), SHAPE), (down(T=0), SHAPE), (down(T=1025), SHAPE),
        (down(I=40), SHAPE), (down(I=256 + 32, dd=G.DT_Q6_K), SHAPE),
        (rt(x=None), NULL), (rt(r=None), NULL), (rt(i=None), NULL), (rt(ww=None), NULL), (rt(off=None), NULL), (rt(pr=None), NULL),
        (rt(K=5), SHAPE), (rt(E=257), SHAPE), (rt(T=0), SHAPE), (rt(T=1025), SHAPE), (rt(K=17, E=32), SHAPE), (rt(H=0), SHAPE),
    ]
    ops.synchronize()
    for n, (got, want) in enumerate(calls):
        assert got == want, (n, got, want)
    for o in (act, y, o_ids, o_w, o_off, o_pairs):
        assert o.untouched()
    # ... and the same buffers take a good call afterwards
    assert gate_up() == 0 and down() == 0 and rt() == 0
    ops.synchronize()
    assert np.abs(y.read().reshape(T, hidden) - c["y"][:T]).max() <= tol_for(c["y"][:T], inter)
    for b in (dx, dres, dids, dw, doff, dpairs, dact_in, part, router):
        b.free()
