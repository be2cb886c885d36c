"""GPU tests of the static decode activations (csrc/gemv.hip: g_decode_arena, the early-x forms of gemv_q8l_kernel) and of the engine option
"static_activations" (include/ntransformer.h).

With x in a static slot the lane-major Q8_0 GEMV requests x before its kernel arguments have arrived: the same loads of the same values, issued
earlier.  So every comparison here is EXACT bit equality against the ordinary kernel on the same inputs, and the form a launch took is read back
(ntk_debug_gemv_static_x) so that a test cannot pass by comparing the ordinary kernel with itself.

Run on the MI355X box:  python -m pytest tests/test_static_activations_gpu.py -m gpu -x -q
"""
import gc

import numpy as np
import pytest

from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from ntransformer_amd import ops
from ntransformer_amd.ops import DeviceBuffer as DB

pytestmark = pytest.mark.gpu

Q8 = G.GGML_TO_DT[G.GGML_Q8_0]
SLOT_FLOATS = {ops.ARENA_HIDDEN: 8192, ops.ARENA_ATTN_OUT: 8192, ops.ARENA_GATE: 32768}   # NTK_ARENA_*_FLOATS


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261020, seed]))


def q8_matrix(r, out_f, in_f):
    """[out_f][in_f] Q8_0 blocks as bytes: quants over the whole int8 range, FP16 scales of both signs over four decades"""
    nb = out_f * in_f // 32
    blk = np.empty((nb, 34), np.uint8)
    d = (r.choice([-1.0, 1.0], nb) * 10.0 ** r.uniform(-5, -1, nb)).astype("<f2")
    blk[:, 0:2] = d.view(np.uint8).reshape(nb, 2)
    blk[:, 2:] = r.integers(-128, 128, (nb, 32), dtype=np.int8).view(np.uint8)
    return blk.reshape(-1)


def launch(packed, rows, in_f, x_ptr, norm_w=None, resid=None, silu_pair=False):
    """one ntk_gemv_rp_fused over the packed matrices with x at x_ptr: (outputs, the early-x slot the launch took)"""
    ys = []
    for i, _ in enumerate(packed):
        y0 = resid if (resid is not None and i == 0) else np.full(rows, np.nan, np.float32)
        ys.append(DB.from_numpy(y0.astype(np.float32)))
    segs = [(W, y, rows, Q8) for W, y in zip(packed, ys)]
    ops.gemv_rp_fused(segs, x_ptr, in_f, norm_w=norm_w, eps=1e-5 if norm_w is not None else 0.0, resid=ys[0] if resid is not None else None,
                      silu_pair=silu_pair)
    form = ops.gemv_static_x()
    ops.synchronize()
    n_out = 1 if silu_pair else len(packed)
    return [y.numpy(np.float32)[:rows].copy() for y in ys[:n_out]], form


def same_bits(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


def case(seed, rows, in_f, n_mats):
    r = rng(seed)
    mats = [ops.q8l_pack(DB.from_numpy(q8_matrix(r, rows, in_f)), rows, in_f) for _ in range(n_mats)]
    x = r.standard_normal(in_f).astype(np.float32)
    x[in_f // 3] *= 50.0
    nw = DB.from_numpy((1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32))
    res = r.standard_normal(rows).astype(np.float32)
    return mats, x, nw, res


def arena_is_free():
    gc.collect()   # (engines other tests dropped without close())
    L = _lib.lib()
    token = L.ntk_decode_arena_acquire()
    if token < 0:
        return False
    L.ntk_decode_arena_release(token)
    return True


def in_slot(slot, x, offset_floats=0):
    """x written into a static slot (the rest of the slot poisoned with NaN): its device address"""
    assert arena_is_free(), "a live engine owns the static decode slots: writing into them would corrupt its state"
    base = ops.decode_arena_slot(slot)
    ops.synchronize()
    ops.upload_to(base, np.full(SLOT_FLOATS[slot], np.nan, np.float32))
    ops.upload_to(base + 4 * offset_floats, x)
    return base + 4 * offset_floats


# ------------------------------------------------------------------------------- the GEMV forms
@pytest.mark.parametrize("rows", [1, 9, 24, 520])   # 9: fewer rows than waves; 520: more than one row per wave
def test_4096_columns_x_in_the_hidden_slot_equals_the_ordinary_kernel(rows):
    mats, x, nw, res = case(rows, rows, 4096, 2)
    outside = DB.from_numpy(x)
    xs = in_slot(ops.ARENA_HIDDEN, x)
    forms = {"plain": dict(), "norm": dict(norm_w=nw), "resid": dict(resid=res), "silu": dict(norm_w=nw, silu_pair=True)}
    for name, kw in forms.items():
        m = mats if name == "silu" else mats[:1]
        want, f0 = launch(m, rows, 4096, outside.ptr, **kw)
        got, f1 = launch(m, rows, 4096, xs, **kw)
        # every reader of the hidden state norms it: the early-x form exists with the fused RMSNorm only; without one the ordinary kernel runs
        assert f0 == 0 and f1 == (ops.ARENA_HIDDEN if "norm_w" in kw else 0), (name, f0, f1)
        assert np.isfinite(got[0]).all() and same_bits(want, got), (name, np.flatnonzero(want[0] != got[0])[:8])


@pytest.mark.parametrize("rows", [1, 9, 24, 520])
def test_4096_columns_x_in_the_attention_output_slot(rows):
    mats, x, nw, res = case(rows + 1000, rows, 4096, 1)
    outside = DB.from_numpy(x)
    xs = in_slot(ops.ARENA_ATTN_OUT, x)
    for name, kw in {"plain": dict(), "resid": dict(resid=res)}.items():
        want, f0 = launch(mats, rows, 4096, outside.ptr, **kw)
        got, f1 = launch(mats, rows, 4096, xs, **kw)
        assert f0 == 0 and f1 == ops.ARENA_ATTN_OUT, (name, f0, f1)
        assert np.isfinite(got[0]).all() and same_bits(want, got), name


@pytest.mark.parametrize("rows", [8, 20])
def test_14336_columns_the_multi_slice_form(rows):
    mats, x, nw, res = case(rows + 2000, rows, 14336, 1)
    outside = DB.from_numpy(x)
    xs = in_slot(ops.ARENA_GATE, x)
    for name, kw in {"resid": dict(resid=res), "plain": dict()}.items():
        want, f0 = launch(mats, rows, 14336, outside.ptr, **kw)
        got, f1 = launch(mats, rows, 14336, xs, **kw)
        assert f0 == 0 and f1 == ops.ARENA_GATE, (name, f0, f1)
        assert np.isfinite(got[0]).all() and same_bits(want, got), name


def test_fallback_x_elsewhere_or_in_the_wrong_slot_takes_the_ordinary_kernel():
    rows = 24
    mats, x, nw, res = case(77, rows, 4096, 2)
    outside = DB.from_numpy(x)
    want = {name: launch(mats if name == "silu" else mats[:1], rows, 4096, outside.ptr, **kw)[0]
            for name, kw in {"resid": dict(resid=res), "norm": dict(norm_w=nw), "silu": dict(norm_w=nw, silu_pair=True)}.items()}
    # the SiLU x up slot has no 4096-column form; the attention-output slot has none with RMSNorm; an address inside a slot is not the slot
    places = [(in_slot(ops.ARENA_GATE, x), ("resid", "norm", "silu")), (in_slot(ops.ARENA_ATTN_OUT, x), ("norm", "silu")),
              (in_slot(ops.ARENA_HIDDEN, x, offset_floats=64), ("resid", "norm", "silu"))]
    for xs, names in places:
        for name in names:
            kw = {"resid": dict(resid=res), "norm": dict(norm_w=nw), "silu": dict(norm_w=nw, silu_pair=True)}[name]
            got, f = launch(mats if name == "silu" else mats[:1], rows, 4096, xs, **kw)
            assert f == 0, (name, f)
            assert same_bits(want[name], got), name
    # 14336 columns from the hidden slot (the hidden and attention-output slots are adjacent: 16384 floats): no such form
    mats, x, nw, res = case(78, 8, 14336, 1)
    outside = DB.from_numpy(x)
    want, _ = launch(mats, 8, 14336, outside.ptr, resid=res)
    base = ops.decode_arena_slot(ops.ARENA_HIDDEN)
    assert ops.decode_arena_slot(ops.ARENA_ATTN_OUT) == base + 4 * SLOT_FLOATS[ops.ARENA_HIDDEN]
    ops.upload_to(base, x)
    got, f = launch(mats, 8, 14336, base, resid=res)
    assert f == 0 and same_bits(want, got)


# ------------------------------------------------------------------------------- the engine
STATIC = "static activations"


def tiny_engine(static=None, shared_from=None):
    e = E.Engine()
    if static is not None:
        e.set_option("static_activations", static)
    if shared_from is not None:
        e.load_shared(shared_from, 64)
    else:
        e.load_synthetic(E.synth_spec("tiny", "Q8_0"), 64)
    return e


def run(e, steps=10):
    """prompt, a few single steps (eager and from the captured graph), a greedy run: (tokens, last-step logits)"""
    prompt = [256, 5, 9, 300]
    lg = e.forward(prompt, 0)
    pos, tok = len(prompt), int(np.argmax(lg))
    toks = []
    for i in range(3):
        lg = e.decode_fused(tok, pos, graph=i == 2)
        pos, tok = pos + 1, int(np.argmax(lg))
        toks.append(tok)
    toks += e.decode_greedy_steps(tok, pos, steps)
    last = e.decode_fused(toks[-2], pos + steps - 1, graph=True)   # the greedy run's last step once more: its logits
    return toks, last


def test_option_on_and_off_give_the_same_tokens_and_logits():
    assert arena_is_free(), "an engine outside this test still owns the static decode slots"
    on = tiny_engine()
    assert STATIC in on.decode_path()
    t_on, l_on = run(on)
    on.close()
    off = tiny_engine(static=0)
    assert STATIC not in off.decode_path() and arena_is_free()
    t_off, l_off = run(off)
    with pytest.raises(_lib.NtkError):
        off.set_option("static_activations", 1)   # after the load
    off.close()
    assert np.isfinite(l_on).all() and t_on == t_off
    assert np.array_equal(l_on.view(np.uint32), l_off.view(np.uint32))
    e = E.Engine()
    with pytest.raises(_lib.NtkError):
        e.set_option("static_activations", "2")
    e.close()


def test_an_engine_with_the_8b_widths_launches_the_early_forms():
    """one layer of 4096 / 14336 columns: the fused path's launches take the early-x forms when the engine owns the slots (read back after the last
    launch of the layer loop -- down, the SiLU x up slot -- and of a whole step -- the LM head, the hidden slot), the ordinary kernel when it does not,
    and both give the same bits"""
    assert arena_is_free(), "an engine outside this test still owns the static decode slots"
    spec = E.SynthSpec(4096, 14336, 1, 32, 8, 512, 64, 1e-5, 500000.0, 256, 257, b"Q8_0", 20261020)
    hidden = rng(5).standard_normal(4096).astype(np.float32)
    out = {}
    for static in (1, 0):
        e = E.Engine()
        e.set_option("static_activations", static)
        e.load_synthetic(spec, 64)
        assert (STATIC in e.decode_path()) == bool(static)
        lg0 = e.forward([256, 5, 9], 0)
        h = e.debug_run_layers(hidden, 3, 0, 1, mode=1)
        f_down = ops.gemv_static_x()
        lg = e.decode_fused(7, 3, graph=False)
        f_head = ops.gemv_static_x()
        lg2 = e.decode_fused(int(np.argmax(lg)), 4, graph=True)
        assert (f_down, f_head) == ((ops.ARENA_GATE, ops.ARENA_HIDDEN) if static else (0, 0)), (static, f_down, f_head)
        out[static] = np.concatenate([lg0, h.reshape(-1), lg, lg2])
        e.close()
    assert np.isfinite(out[1]).all() and np.array_equal(out[1].view(np.uint32), out[0].view(np.uint32))


def test_one_owner_per_process_second_engine_and_shared_sequence_run_on_their_own_buffers():
    assert arena_is_free(), "an engine outside this test still owns the static decode slots"
    solo = tiny_engine(static=0)
    t_solo, l_solo = run(solo)
    solo.close()
    owner = tiny_engine()
    second = tiny_engine()
    shared = tiny_engine(shared_from=owner)
    assert STATIC in owner.decode_path() and STATIC not in second.decode_path() and STATIC not in shared.decode_path()
    results = [run(owner), run(second), run(shared), run(owner)]   # (interleaved: the owner's slots hold only its own state)
    for toks, last in results:
        assert toks == t_solo and np.array_equal(last.view(np.uint32), l_solo.view(np.uint32))
    shared.close()
    owner.close()
    assert STATIC not in second.decode_path()   # ownership is decided at load
    third = tiny_engine()                        # the owner has closed: the next engine to load takes the slots
    assert STATIC in third.decode_path()
    toks, last = run(third)
    assert toks == t_solo and np.array_equal(last.view(np.uint32), l_solo.view(np.uint32))
    third.close()
    second.close()
    assert arena_is_free()
