"""GPU tests of the lane-major Q8_0 repack and the decode GEMV that reads it (csrc/gemv.hip, layout: csrc/gemv_core.hip.h / DESIGN 2).

The pack / unpack entry points are ntk_q8l_bytes / ntk_q8l_pack / ntk_q8l_unpack: ntk_rp_bytes / ntk_rp_pack keep refusing Q8_0, which
tests/test_gemv_rp.py pins.  The layout is pinned by a NumPy packer written here from its description; the kernel over the packed rows must give the SAME BITS as the
kernel over the GGUF blocks (the same dwords through the same arithmetic in the same order: only the transport differs), in every form the
engine launches; and the engine with the repack on and off must give the same logits bits and the same greedy stream.

Run on the MI355X box:  python -m pytest tests/test_gemv_q8_lane_major.py -m gpu -x -q
"""
import numpy as np
import pytest

from ntransformer_amd import _lib
from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from ntransformer_amd import ops
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O
from test_oracle_golden import golden_model

pytestmark = pytest.mark.gpu

Q8 = G.GGML_TO_DT[G.GGML_Q8_0]
Q4K = G.GGML_TO_DT[G.GGML_Q4_K]
NOT_TAKEN = (-1, -2, -4)   # NTK_E_DTYPE / NTK_E_SHAPE / NTK_E_ALIGN: "nothing was launched, try the next form"


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261017, seed]))


def tol_for(y, in_f):
    # the tolerance of the Q8_0 GEMV tests in tests/test_hip_kernels.py
    return 4e-6 * np.sqrt(in_f) * max(1.0, float(np.abs(y).max()))


def q8_matrix(r, out_f, in_f):
    """[out_f][in_f] Q8_0 blocks as bytes: quants over the whole int8 range, FP16 scales of both signs over four decades"""
    nb = out_f * in_f // 32
    blk = np.empty((nb, 34), np.uint8)
    d = (r.choice([-1.0, 1.0], nb) * 10.0 ** r.uniform(-5, -1, nb)).astype("<f2")
    blk[:, 0:2] = d.view(np.uint8).reshape(nb, 2)
    blk[:, 2:] = r.integers(-128, 128, (nb, 32), dtype=np.int8).view(np.uint8)
    return blk.reshape(-1)


def slices_of(in_f):
    """the column slices of a row of in_f columns: (number, width) -- the launcher's rule, restated"""
    ns = (in_f + 4095) // 4096
    per = (in_f + ns - 1) // ns
    return ns, (per + 63) // 64 * 64


def numpy_pack(W, out_f, in_f):
    """the lane-major layout from its description: per row and slice of nl lanes, chunk j of lane l at (j nl + l) 16, scales at 64 nl + 4 l"""
    ns, width = slices_of(in_f)
    rows = W.reshape(out_f, in_f // 32, 34)
    out = np.empty((out_f, in_f // 32 * 34), np.uint8)
    for s in range(ns):
        c0, c1 = s * width, min(in_f, (s + 1) * width)
        nl = (c1 - c0) // 64
        blk = rows[:, c0 // 32:c1 // 32, :]                                   # [rows][2 nl][34]
        quants = blk[:, :, 2:].reshape(out_f, nl, 4, 16)                      # [rows][lane][chunk][16]
        scales = blk[:, :, :2].reshape(out_f, nl, 4)                          # [rows][lane][d(2l) lo, hi, d(2l+1) lo, hi]
        base = c0 // 32 * 34
        out[:, base:base + 64 * nl] = quants.transpose(0, 2, 1, 3).reshape(out_f, 64 * nl)
        out[:, base + 64 * nl:base + 68 * nl] = scales.reshape(out_f, 4 * nl)
    return out.reshape(-1)


# ------------------------------------------------------------------------------- the layout
@pytest.mark.parametrize("out_f,in_f", [(8, 256), (5, 512), (64, 4096), (3, 8192), (16, 14336)])
def test_pack_is_the_described_layout_and_unpack_its_inverse(out_f, in_f):
    W = q8_matrix(rng(out_f + in_f), out_f, in_f)
    assert ops.q8l_bytes(out_f, in_f) == W.size                # the same bytes, permuted
    rp = ops.q8l_pack(DB.from_numpy(W), out_f, in_f)
    got = rp.numpy(np.uint8)[:W.size]
    want = numpy_pack(W, out_f, in_f)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    back = ops.q8l_unpack(rp, out_f, in_f, W.size).numpy(np.uint8)[:W.size]
    assert np.array_equal(back, W), int((back != W).sum())


# ------------------------------------------------------------------------------- the kernel: same bits as over the GGUF blocks
def both(segs_raw, x, in_f, **kw):
    """ntk_gemv_fused over GGUF blocks and ntk_gemv_rp_fused over their packed form: segs_raw = [(W bytes, rows)], outputs as lists"""
    xd = DB.from_numpy(x)
    nwd = DB.from_numpy(kw["norm_w"]) if kw.get("norm_w") is not None else None
    outs = []
    for packed in (False, True):
        ys, segs, keep = [], [], []
        for W, rows in segs_raw:
            Wd = DB.from_numpy(W)
            if packed:
                Wd = ops.q8l_pack(Wd, rows, in_f)
            keep.append(Wd)
            y0 = kw["resid"] if kw.get("resid") is not None and not ys else np.full(rows, np.nan, np.float32)
            ys.append(DB.from_numpy(y0.astype(np.float32)))
            segs.append((Wd, ys[-1], rows, Q8))
        args = dict(norm_w=nwd, eps=1e-5 if nwd is not None else 0.0, resid=ys[0] if kw.get("resid") is not None else None,
                    silu_pair=bool(kw.get("silu_pair")))
        (ops.gemv_rp_fused if packed else ops.gemv_fused)(segs, xd, in_f, **args)
        ops.synchronize()
        outs.append([y.numpy(np.float32)[:rows].copy() for y, (_, rows) in zip(ys, segs_raw)])
    return outs


def same_bits(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


@pytest.mark.parametrize("in_f", [256, 4096, 14336])
@pytest.mark.parametrize("out_f", [1, 7, 520, 4100])
def test_plain_and_norm_forms_equal_the_raw_kernel_bit_for_bit_and_the_oracle(out_f, in_f):
    r = rng(out_f * 3 + in_f)
    W = q8_matrix(r, out_f, in_f)
    x = r.standard_normal(in_f).astype(np.float32)
    x[in_f // 3] *= 50.0
    raw, lm = both([(W, out_f)], x, in_f)
    assert np.isfinite(lm[0]).all() and same_bits(raw, lm), np.flatnonzero(raw[0] != lm[0])[:8]
    ref = O.gemv(W, x, out_f, in_f, Q8)
    assert np.abs(lm[0] - ref).max() <= tol_for(ref, in_f), np.abs(lm[0] - ref).max()
    nw = (1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32)
    raw, lm = both([(W, out_f)], x, in_f, norm_w=nw)
    assert np.isfinite(lm[0]).all() and same_bits(raw, lm), np.flatnonzero(raw[0] != lm[0])[:8]
    ref = O.gemv(W, O.rmsnorm(x, nw, 1e-5).reshape(-1), out_f, in_f, Q8)
    assert np.abs(lm[0] - ref).max() <= tol_for(ref, in_f), np.abs(lm[0] - ref).max()


@pytest.mark.parametrize("in_f", [256, 4096, 14336])
def test_three_unequal_segments_sharing_x(in_f):
    r = rng(in_f + 11)
    mats = [(q8_matrix(r, n, in_f), n) for n in (96, 32, 32)]
    x = r.standard_normal(in_f).astype(np.float32)
    nw = (1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32)
    for kw in ({}, {"norm_w": nw}):
        raw, lm = both(mats, x, in_f, **kw)
        assert all(np.isfinite(y).all() for y in lm) and same_bits(raw, lm)


@pytest.mark.parametrize("in_f", [256, 4096, 14336])
@pytest.mark.parametrize("out_f", [1, 7, 520, 4100])
def test_residual_added_in_place(out_f, in_f):
    r = rng(out_f * 5 + in_f)
    W = q8_matrix(r, out_f, in_f)
    x = r.standard_normal(in_f).astype(np.float32)
    res = r.standard_normal(out_f).astype(np.float32)
    raw, lm = both([(W, out_f)], x, in_f, resid=res)
    assert np.isfinite(lm[0]).all() and same_bits(raw, lm)
    assert not np.array_equal(lm[0], res)


@pytest.mark.parametrize("in_f", [256, 4096, 14336])
@pytest.mark.parametrize("out_f", [1, 7, 520, 4100])
def test_silu_pair(out_f, in_f):
    r = rng(out_f * 7 + in_f)
    Wg, Wu = q8_matrix(r, out_f, in_f), q8_matrix(r, out_f, in_f)
    x = r.standard_normal(in_f).astype(np.float32)
    nw = (1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32)
    raw, lm = both([(Wg, out_f), (Wu, out_f)], x, in_f, norm_w=nw, silu_pair=True)
    assert np.isfinite(lm[0]).all() and same_bits(raw[:1], lm[:1])


# ------------------------------------------------------------------------------- not taken
def test_shapes_and_mixes_outside_the_format_are_not_taken(tmp_path):
    L = _lib.lib()
    assert ops.q8l_bytes(4, 288) == 0                                  # one slice of 288 columns: not a multiple of 256
    d, x, y, y2 = DB.zeros(1 << 16), DB.zeros(4 * 512), DB.zeros(64), DB.zeros(64)
    assert L.ntk_q8l_pack(d.ptr, d.ptr, 4, 288, None) in NOT_TAKEN
    one = (_lib.GemvSeg * 1)()
    one[0].W, one[0].y, one[0].rows, one[0].dtype = d.ptr, y.ptr, 4, Q8
    assert L.ntk_gemv_rp_fused(one, 1, x.ptr, 288, None, 0.0, None, 0, None) in NOT_TAKEN
    segs = (_lib.GemvSeg * 2)()
    for i, (yy, dt) in enumerate(((y, Q8), (y2, Q4K))):
        segs[i].W, segs[i].y, segs[i].rows, segs[i].dtype = d.ptr, yy.ptr, 16, dt
    assert L.ntk_gemv_rp_fused(segs, 2, x.ptr, 256, None, 0.0, None, 0, None) in NOT_TAKEN
    # through the engine: a Q8_0 model whose down projection has 384 columns (one slice, not a multiple of 256; a width the prompt GEMM takes) decodes,
    # that matrix on the raw path, with the same bits as without any repack
    assert ops.q8l_bytes(256, 384) == 0
    shape = G.LlamaShape("odd", 256, 384, 2, 4, 2, 512, ctx=64, bos=256, eos=257)
    path = str(tmp_path / "odd_q8_0.gguf")
    G.make_synthetic_llama(path, shape, "Q8_0", seed=7)
    outs = {}
    for level in (0, 3):
        eng = E.Engine()
        eng.set_option("repack", level)
        eng.load(path, 64)
        lg = [eng.forward([256, 5, 9, 300], 0)]
        for i in range(3):
            lg.append(eng.decode_fused(int(np.argmax(lg[-1])), 4 + i, graph=i == 2))
        outs[level] = np.stack(lg)
        if level:
            assert 0 < eng.repacked_bytes() < eng.weight_bytes()
        eng.close()
    assert np.isfinite(outs[3]).all() and np.array_equal(outs[0], outs[3])
    m = O.OracleModel(path, 64)
    assert np.abs(outs[3][0] - m.forward([256, 5, 9, 300], 0)).max() <= 1e-3


# ------------------------------------------------------------------------------- the engine
@pytest.mark.parametrize("name,shape", [("tiny_q8_0", G.TINY), ("small_q8_0", G.SMALL)])
def test_engine_gives_the_same_bits_with_the_repack_on_and_off(name, shape, tmp_path):
    path, z = golden_model(name, shape, "Q8_0", tmp_path)
    prompt = [int(t) for t in z["prompt"]]
    fed = [int(t) for t in z["fed"][1:]][:6]
    logits, streams, resident = {}, {}, {}
    for level in (0, 3):
        eng = E.Engine()
        eng.set_option("repack", level)
        eng.load(path, int(z["ctx"]))
        lg = [eng.forward(prompt, 0)]                       # the prompt pass reads the GGUF bytes that stay beside the repack ...
        pos = len(prompt)
        for i, t in enumerate(fed):                         # ... and the decode steps behind it alternate eager / hipGraph
            lg.append(eng.decode_fused(t, pos, graph=i % 2 == 1))
            pos += 1
        lg.append(eng.forward(prompt, 0))                   # a prompt pass AFTER decode steps: the GGUF bytes are still what they were
        logits[level] = np.stack(lg)
        streams[level] = eng.decode_greedy_steps(int(np.argmax(lg[-1])), len(prompt), 12)
        resident[level] = (eng.resident_weight_bytes(), eng.weight_bytes(), eng.repacked_bytes())
        eng.close()
    assert np.isfinite(logits[3]).all()
    assert np.array_equal(logits[0].view(np.uint32), logits[3].view(np.uint32)), float(np.abs(logits[0] - logits[3]).max())
    assert streams[0] == streams[3]
    assert np.abs(logits[3][0] - z["logits"][0]).max() <= 1e-3   # (the golden logits of the prompt: the reference's host code)
    res0, w0, rp0 = resident[0]
    res3, w3, rp3 = resident[3]
    assert rp0 == 0 and res0 == w0
    assert rp3 > 0 and res3 == w3 + rp3                     # both copies are resident and reported
