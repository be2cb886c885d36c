"""GPU tests of the lane-major Q8_0 decode GEMV on rows of SEVERAL column slices (csrc/gemv.hip: the NS_SPLIT instantiations of gemv_q8l_kernel,
one wave per slice, partial sums combined through LDS, the segment table of that step in scalar registers) -- 2, 3 and 4 slices, full and
56-lane slices, 1 row to more than two rows per wave.

The kernel over the packed rows (ntk_gemv_rp_fused) must give the SAME BITS as the kernel over the GGUF blocks (ntk_gemv_fused): the same
per-slice totals added in slice order from 0.0f, the same epilogues.  Every output buffer is poisoned with NaN before the call (a row never
stored shows), rows of 28672 columns (7 slices, the image built in two passes) are covered too, and the engine gives the same logits with the
repack on and off.

One matrix per row width is generated, uploaded and packed once; the cases take their rows from it (a row's packed bytes do not depend on
the rows around it), and the oracle's results for all of its rows are computed once.

Run on the MI355X box:  python -m pytest tests/test_gemv_q8_multi_slice.py -m gpu -x -q
"""
import numpy as np
import pytest

from ntransformer_amd import engine as E
from ntransformer_amd import gguf as G
from ntransformer_amd import ops
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O
from test_oracle_golden import golden_model

pytestmark = pytest.mark.gpu

Q8 = G.GGML_TO_DT[G.GGML_Q8_0]
# 8192: 2 slices of 4096; 12288: 3 slices, all 64 lanes; 14336: 4 slices of 3584, 56 live lanes; 16384: 4 slices of 4096
WIDTHS = [8192, 12288, 14336, 16384]
# 1, 7: most waves without a row, one partial batch; 4100: 2..5 rows per wave depending on the slice count (at 4 slices a full batch of 4 and a
# partial one behind it); 8200: 4..9 rows -- two full batches, both register sets, both halves of the partial-sum buffer
ROWS = [1, 7, 4100, 8200]
MAX_ROWS = max(ROWS)
UP_AT = 100          # silu_pair: the "up" matrix is rows UP_AT .. of the same pool (gate row i meets pool row UP_AT + i)


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(seed):
    return np.random.Generator(np.random.Philox(key=[20261018, seed]))


def tol_for(y, in_f):
    # the tolerance of the Q8_0 GEMV tests in tests/test_hip_kernels.py and tests/test_gemv_q8_lane_major.py
    return 4e-6 * np.sqrt(in_f) * max(1.0, float(np.abs(y).max()))


def q8_matrix(r, out_f, in_f):
    """[out_f][in_f] Q8_0 blocks as bytes: quants over the whole int8 range, FP16 scales of both signs over four decades"""
    nb = out_f * in_f // 32
    blk = np.empty((nb, 34), np.uint8)
    d = (r.choice([-1.0, 1.0], nb) * 10.0 ** r.uniform(-5, -1, nb)).astype("<f2")
    blk[:, 0:2] = d.view(np.uint8).reshape(nb, 2)
    blk[:, 2:] = r.integers(-128, 128, (nb, 32), dtype=np.int8).view(np.uint8)
    return blk.reshape(-1)


class Pool:
    """MAX_ROWS + UP_AT rows of one width: GGUF bytes and their lane-major pack on the device, x, norm weights, the oracle's results"""

    def __init__(self, in_f):
        r = rng(in_f)
        self.in_f, self.rows = in_f, MAX_ROWS + UP_AT
        self.row_bytes = in_f // 32 * 34
        W = q8_matrix(r, self.rows, in_f)
        self.x = r.standard_normal(in_f).astype(np.float32)
        self.x[in_f // 3] *= 50.0
        self.nw = (1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32)
        self.res = r.standard_normal(MAX_ROWS).astype(np.float32)
        self.ref = O.gemv(W, self.x, MAX_ROWS, in_f, Q8)
        self.ref_norm = O.gemv(W, O.rmsnorm(self.x, self.nw, 1e-5).reshape(-1), MAX_ROWS, in_f, Q8)
        self.raw = DB.from_numpy(W)
        self.packed = ops.q8l_pack(self.raw, self.rows, in_f)
        self.xd, self.nwd = DB.from_numpy(self.x), DB.from_numpy(self.nw)

    def run(self, segs, norm=False, resid=False, silu_pair=False):
        """segs = [(first pool row, rows)]: the call over the GGUF bytes and over the packed rows; every output starts as NaN (or the residual)"""
        outs = []
        for packed in (False, True):
            base = (self.packed if packed else self.raw).ptr
            ys, sg = [], []
            for i, (r0, n) in enumerate(segs):
                y0 = self.res[:n] if resid and i == 0 else np.full(n, np.nan, np.float32)
                ys.append(DB.from_numpy(y0))
                sg.append((base + r0 * self.row_bytes, ys[-1], n, Q8))
            (ops.gemv_rp_fused if packed else ops.gemv_fused)(sg, self.xd, self.in_f, norm_w=self.nwd if norm else None,
                                                              eps=1e-5 if norm else 0.0, resid=ys[0] if resid else None, silu_pair=silu_pair)
            ops.synchronize()
            outs.append([y.numpy(np.float32)[:n].copy() for y, (_, n) in zip(ys, segs)])
        return outs


@pytest.fixture(scope="module", params=WIDTHS)
def pool(request):
    p = Pool(request.param)
    yield p
    del p


def same_bits(a, b):
    return all(np.array_equal(u.view(np.uint32), v.view(np.uint32)) for u, v in zip(a, b))


@pytest.mark.parametrize("out_f", ROWS)
def test_plain_and_norm_forms_equal_the_raw_kernel_bit_for_bit_and_the_oracle(pool, out_f):
    for norm, ref in ((False, pool.ref), (True, pool.ref_norm)):
        raw, lm = pool.run([(0, out_f)], norm=norm)
        assert np.isfinite(lm[0]).all() and same_bits(raw, lm), np.flatnonzero(raw[0] != lm[0])[:8]
        err = np.abs(lm[0] - ref[:out_f]).max()
        assert err <= tol_for(ref[:out_f], pool.in_f), err


@pytest.mark.parametrize("out_f", ROWS)
def test_residual_added_in_place(pool, out_f):
    raw, lm = pool.run([(0, out_f)], resid=True)
    assert np.isfinite(lm[0]).all() and same_bits(raw, lm), np.flatnonzero(raw[0] != lm[0])[:8]
    assert not np.array_equal(lm[0], pool.res[:out_f])


@pytest.mark.parametrize("out_f", ROWS)
def test_silu_pair(pool, out_f):
    for norm in (True, False):
        raw, lm = pool.run([(0, out_f), (UP_AT, out_f)], norm=norm, silu_pair=True)
        assert np.isfinite(lm[0]).all() and same_bits(raw[:1], lm[:1]), np.flatnonzero(raw[0] != lm[0])[:8]


@pytest.mark.parametrize("out_f", ROWS[1:])      # (three segments need three rows)
def test_three_unequal_segments_sharing_x(pool, out_f):
    a, b = out_f // 2 + 1, out_f // 3
    segs = [(0, a), (a, b), (a + b, out_f - a - b)]
    for norm, ref in ((False, pool.ref), (True, pool.ref_norm)):
        raw, lm = pool.run(segs, norm=norm)
        assert all(np.isfinite(y).all() for y in lm) and same_bits(raw, lm)
        assert np.abs(np.concatenate(lm) - ref[:out_f]).max() <= tol_for(ref[:out_f], pool.in_f)


# ------------------------------------------------------------------------------- 7 slices: the activation image in two passes
@pytest.mark.parametrize("out_f", [7, 520])
def test_rows_of_28672_columns_keep_the_raw_kernels_bits(out_f):
    in_f = 28672
    r = rng(out_f + in_f)
    W = q8_matrix(r, 2 * out_f, in_f)
    x = r.standard_normal(in_f).astype(np.float32)
    res = r.standard_normal(out_f).astype(np.float32)
    rb = in_f // 32 * 34
    raw = DB.from_numpy(W)
    packed = ops.q8l_pack(raw, 2 * out_f, in_f)
    xd = DB.from_numpy(x)
    ref = O.gemv(W, x, out_f, in_f, Q8)
    a, b = out_f // 2 + 1, out_f // 3
    forms = {"plain": ([(0, out_f)], {}), "resid": ([(0, out_f)], {"resid": True}), "silu": ([(0, out_f), (out_f, out_f)], {"silu_pair": True}),
             "segments": ([(0, a), (a, b), (a + b, out_f - a - b)], {})}
    for name, (segs, kw) in forms.items():
        got = []
        for fn, base in ((ops.gemv_fused, raw.ptr), (ops.gemv_rp_fused, packed.ptr)):
            ys = [DB.from_numpy(res[:n] if kw.get("resid") and i == 0 else np.full(n, np.nan, np.float32)) for i, (_, n) in enumerate(segs)]
            fn([(base + r0 * rb, y, n, Q8) for y, (r0, n) in zip(ys, segs)], xd, in_f, resid=ys[0] if kw.get("resid") else None,
               silu_pair=bool(kw.get("silu_pair")))
            ops.synchronize()
            got.append([y.numpy(np.float32)[:n].copy() for y, (_, n) in zip(ys, segs)])
        keep = 1 if name == "silu" else len(segs)
        assert all(np.isfinite(y).all() for y in got[1][:keep]) and same_bits(got[0][:keep], got[1][:keep]), name
        if name in ("plain", "segments"):
            assert np.abs(np.concatenate(got[1]) - ref).max() <= tol_for(ref, in_f), name


# ------------------------------------------------------------------------------- the engine
@pytest.mark.parametrize("name,shape", [("tiny_q8_0", G.TINY), ("small_q8_0", G.SMALL)])
def test_engine_gives_the_same_logits_with_repack_1_and_0(name, shape, tmp_path):
    path, z = golden_model(name, shape, "Q8_0", tmp_path)
    prompt = [int(t) for t in z["prompt"]]
    fed = [int(t) for t in z["fed"][1:]][:6]
    logits, streams = {}, {}
    for level in (0, 1):
        eng = E.Engine()
        eng.set_option("repack", level)
        eng.load(path, int(z["ctx"]))
        lg = [eng.forward(prompt, 0)]
        pos = len(prompt)
        for i, t in enumerate(fed):                         # decode steps alternate eager / hipGraph
            lg.append(eng.decode_fused(t, pos, graph=i % 2 == 1))
            pos += 1
        logits[level] = np.stack(lg)
        streams[level] = eng.decode_greedy_steps(int(np.argmax(lg[-1])), len(prompt), 12)
        if level:
            assert eng.repacked_bytes() > 0
        eng.close()
    assert np.isfinite(logits[1]).all()
    assert np.array_equal(logits[0].view(np.uint32), logits[1].view(np.uint32)), float(np.abs(logits[0] - logits[1]).max())
    assert streams[0] == streams[1]
    assert np.abs(logits[1][0] - z["logits"][0]).max() <= 1e-3   # (the golden logits of the prompt: the reference's host code)
