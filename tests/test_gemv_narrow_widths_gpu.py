"""GPU tests of the decode GEMV (csrc/gemv.hip, gemv_core.hip.h) at Q8_0 / Q4_0 widths that are NOT multiples of 256 columns.

Q8_0 and Q4_0 blocks are 32 columns wide and the library takes any multiple of 32 (prepare_quant: in % F::BW; gemv_slices rounds slices to 64
columns), real checkpoints have such widths (896, 11008, 13824, 18944), and every other GEMV test uses multiples of 256.  A lane owns 64 columns
of its slice, so at these widths the kernel runs what it never runs elsewhere: a lane with 32 of its 64 columns (`ncols == 32`: have_hi, the
`ncols > 32 * h` guards of Dot<Q8_0> / Dot<Q4_0>, Q4_0's sx32[h] of a half-empty lane), a last slice shorter than the others that ends in such a
lane, row pitches of 34 k / 18 k bytes that land on every 2-byte residue of a 16-byte chunk, the clamped x / norm-weight loads and the `dummy`
image slot of a row that ends inside a thread's float4 stride.

Geometry of every width below, from gemv_slices(in, 64) -- ns = ceil(in / 4096), slice = ceil(in / ns) rounded up to 64:
  32, 96, 160                 1 slice: one half lane only; full lanes + a half lane; rows of 34 / 102 / 170 bytes (Q8_0)
  320, 864, 2080, 4064        1 slice: 5 lanes; 13.5; 32.5; 63.5 lanes
  4128                        2 x 2112, last 2016: a ragged last slice ending in a half lane
  4160                        2 x 2112, last 2048: ragged, whole lanes
  8224                        3 x 2752, last 2720: 6-wave workgroups, 42.5 lanes
  11008, 13824                3 x 3712 (last 3584); 4 x 3456: multiples of 256 without a lane-major form
  16416                       5 x 3328, last 3104: one row group per workgroup, 5 waves, second image pass with a ragged slice
  28704, 32736                8 slices, last 3168 / 4064: both image passes, the widest rows

The oracle is oracle.gemv (+ oracle.rmsnorm / oracle.silu_mul for the fused forms); the bounds are those of tests/test_hip_kernels.py: tol_for,
x 2 behind the fused norm, x 4 behind SiLU.  Every output buffer starts as NaN (or as the residual) and must come out finite.

Run on the MI355X box:  python -m pytest tests/test_gemv_narrow_widths_gpu.py -m gpu -x -q
"""
import numpy as np
import pytest

from ntransformer_amd import _lib
from ntransformer_amd import gguf as G
from ntransformer_amd import ops
from ntransformer_amd.ops import DeviceBuffer as DB
from oracle import oracle as O
from test_hip_kernels import tol_for

pytestmark = pytest.mark.gpu

QUANT = {"Q8_0": G.GGML_Q8_0, "Q4_0": G.GGML_Q4_0}
WIDTHS = [32, 96, 160, 320, 864, 2080, 4064, 4128, 4160, 8224, 11008, 13824, 16416, 28704, 32736]
POISONED = (32, 96, 2080, 4128)      # widths whose launch follows one that leaves NaN patterns in LDS
FUSED_WIDTHS = [96, 320, 864, 2080, 4128, 8224, 16416]
NOT_TAKEN = (-1, -2, -4)             # NTK_E_DTYPE / NTK_E_SHAPE / NTK_E_ALIGN: "nothing was launched, try the next form"
NTK_E_SHAPE = -2


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


def rng(*key):
    return np.random.Generator(np.random.Philox(key=[20261020, sum(int(k) * 1000003 ** i for i, k in enumerate(key)) & 0xFFFFFFFFFFFFFFFF]))


def slices_of(in_f):
    """gemv_slices(in, 64), restated: (slices, slice width, width of the last slice)"""
    ns = (in_f + 4095) // 4096
    sc = ((in_f + ns - 1) // ns + 63) // 64 * 64
    return ns, sc, in_f - (ns - 1) * sc


def test_the_widths_have_the_geometry_the_cases_are_chosen_for():
    """(no kernel: the table in the module docstring, checked against the launcher's slicing rule)"""
    assert all(w % 32 == 0 and w % 256 != 0 or w in (11008, 13824) for w in WIDTHS)
    assert [slices_of(w)[0] for w in (32, 96, 160, 320, 864, 2080, 4064)] == [1] * 7
    assert [w % 64 for w in (32, 96, 160, 864, 2080, 4064)] == [32] * 6 and 320 % 64 == 0       # a half lane ends the row
    assert slices_of(4128) == (2, 2112, 2016) and 2016 % 64 == 32
    assert slices_of(4160) == (2, 2112, 2048)
    assert slices_of(8224) == (3, 2752, 2720) and 2720 % 64 == 32
    assert slices_of(11008) == (3, 3712, 3584) and slices_of(13824) == (4, 3456, 3456) and 3712 % 256 and 3456 % 256
    assert slices_of(16416) == (5, 3328, 3104) and 3104 % 64 == 32
    assert slices_of(28704) == (8, 3648, 3168) and slices_of(32736) == (8, 4096, 4064)
    assert slices_of(32800)[0] == 9                                                              # refused: more than 8 slices


def matrix(r, qname, rows, in_f):
    return np.frombuffer(G.synth_tensor(r, QUANT[qname], rows, in_f), np.uint8)


def on_device(W):
    """W with 64 all-ones bytes behind it: the kernel reads whole 16-byte chunks, up to 15 bytes past a row that ends off a 16-byte boundary"""
    return DB.from_numpy(np.concatenate([W, np.full(64, 0xFF, np.uint8)]))


def leave_nan_in_lds():
    """One Q8_0 launch of 4096 columns x 512 rows whose weight bytes are all ones (every block scale an FP16 NaN) and whose x is NaN: its
    workgroups leave NaN patterns in their CUs' staging areas and activation image.  The output is ignored."""
    Wd = DB.from_numpy(np.full(512 * 4096 // 32 * 34 + 64, 0xFF, np.uint8))
    xd = DB.from_numpy(np.full(4096, np.nan, np.float32))
    yd = DB.zeros(512 * 4)
    ops.launch_gemv(yd, Wd, xd, 512, 4096, G.DT_Q8_0)
    ops.synchronize()


def gemv_gpu(Wraw, x, out_f, in_f, dt, w_offset=0, poison=False):
    """ntk_gemv into a NaN buffer, W `w_offset` bytes into its allocation; the bytes in front of W and the 64 behind it are all ones (as a block
    scale: an FP16 NaN), so whatever the kernel reads beside the last row's end must not reach a sum"""
    Wb = np.full(Wraw.nbytes + w_offset + 64, 0xFF, np.uint8)
    Wb[w_offset:w_offset + Wraw.nbytes] = Wraw
    Wd = DB.from_numpy(Wb)
    xd = DB.from_numpy(x.astype(np.float32))
    yd = DB.from_numpy(np.full(out_f, np.nan, np.float32))
    if poison: leave_nan_in_lds()
    ops.launch_gemv(yd, Wd.at(w_offset), xd, out_f, in_f, dt)
    ops.synchronize()
    return yd.numpy(np.float32)


def rows_for(in_f):
    return (1, 7, 37, 520) if in_f <= 4160 else (1, 7, 37)


# ------------------------------------------------------------------------------- (1) + (4) ntk_gemv against the oracle
@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("in_f,out_f", [(w, n) for w in WIDTHS for n in rows_for(w)])
def test_gemv_matches_oracle(qname, in_f, out_f):
    """ntk_gemv against oracle.gemv within tol_for at every width of the table: one row (7 of 8 waves without one), 7, 37 (a partial batch in some row
    groups), 520 (a second row per wave: the prefetch) up to 4160 columns.
    At 32 / 96 / 2080 / 4128 columns the launch directly follows leave_nan_in_lds(): LDS is not cleared between launches, so a lane that multiplied
    the stale bytes of its dead half (or of a dead lane) by a zero activation would give NaN.  That part is best-effort by nature -- the launch
    under test need not land on a CU the poisoning launch used, nor on its LDS addresses -- and can only ever fail for a real defect."""
    dt = G.GGML_TO_DT[QUANT[qname]]
    r = rng(in_f, out_f, dt)
    W = matrix(r, qname, out_f, in_f)
    x = r.standard_normal(in_f).astype(np.float32)
    ref = O.gemv(W, x, out_f, in_f, dt)
    y = gemv_gpu(W, x, out_f, in_f, dt, poison=in_f in POISONED)
    assert np.isfinite(y).all()
    err = float(np.abs(y - ref).max())
    print("gemv %s in=%d rows=%d: max err %.3g, bound %.3g" % (qname, in_f, out_f, err, tol_for(ref, in_f)))
    assert err <= tol_for(ref, in_f), err


@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("in_f", [96, 864, 4128])
@pytest.mark.parametrize("off", [2, 6, 14])
def test_gemv_unaligned_weights(qname, in_f, off):
    """W 2 / 6 / 14 bytes into its allocation: with row pitches of 34 k / 18 k bytes every 2-byte residue of a 16-byte chunk starts some row"""
    dt = G.GGML_TO_DT[QUANT[qname]]
    out_f = 37
    r = rng(in_f, off, dt, 1)
    W = matrix(r, qname, out_f, in_f)
    x = r.standard_normal(in_f).astype(np.float32)
    ref = O.gemv(W, x, out_f, in_f, dt)
    y = gemv_gpu(W, x, out_f, in_f, dt, w_offset=off)
    assert np.isfinite(y).all()
    err = float(np.abs(y - ref).max())
    print("gemv %s in=%d w_off=%d: max err %.3g, bound %.3g" % (qname, in_f, off, err, tol_for(ref, in_f)))
    assert err <= tol_for(ref, in_f), err


# ------------------------------------------------------------------------------- (2) ntk_gemv_fused against the oracle's composition
def fused_inputs(r, in_f):
    """x and the norm weights with one float in front: [1:] starts 4 bytes into the (16-byte aligned) allocation"""
    x = (r.standard_normal(in_f + 1) * 3).astype(np.float32)
    nw = (1 + 0.05 * r.uniform(-1, 1, in_f + 1)).astype(np.float32)
    return x, nw


@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("x_off", [0, 4])
@pytest.mark.parametrize("rows", [(40, 8, 8), (320, 64, 64)])
@pytest.mark.parametrize("in_f", FUSED_WIDTHS)
def test_gemv_fused_norm_three_segments(qname, in_f, rows, x_off):
    """RMSNorm prologue + three segments sharing x (Q | K | V) within 2 tol_for; x_off = 4: x and the norm weights 4 bytes off a 16-byte boundary,
    the prologue with plain loops.  At 16416 columns the norm weights no longer fit the fast prologue's registers (in > 4 * 4 * 64 * 5 waves)."""
    dt = G.GGML_TO_DT[QUANT[qname]]
    r = rng(in_f, rows[0], x_off, dt, 2)
    x, nw = fused_inputs(r, in_f)
    o = x_off // 4
    Ws = [matrix(r, qname, n, in_f) for n in rows]
    xn = O.rmsnorm(x[o:o + in_f], nw[o:o + in_f], 1e-5).reshape(-1)
    refs = [O.gemv(W, xn, n, in_f, dt) for W, n in zip(Ws, rows)]
    xd, nd = DB.from_numpy(x), DB.from_numpy(nw)
    Wd = [on_device(W) for W in Ws]
    yd = [DB.from_numpy(np.full(n, np.nan, np.float32)) for n in rows]
    ops.gemv_fused([(Wd[i], yd[i], rows[i], dt) for i in range(3)], xd.at(x_off), in_f, norm_w=nd.at(x_off), eps=1e-5)
    ops.synchronize()
    for i in range(3):
        y = yd[i].numpy()
        assert np.isfinite(y).all()
        err = float(np.abs(y - refs[i]).max())
        print("norm_seg3 %s in=%d rows=%d x_off=%d: max err %.3g, bound %.3g" % (qname, in_f, rows[i], x_off, err, 2 * tol_for(refs[i], in_f)))
        assert err <= 2 * tol_for(refs[i], in_f), (i, err)


@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("x_off", [0, 4])
@pytest.mark.parametrize("in_f", FUSED_WIDTHS)
def test_gemv_fused_residual_in_place(qname, in_f, x_off):
    """hidden += W . x in place (the Wo / down projections; several slices: the cross-slice combine adds the residual) within tol_for"""
    dt = G.GGML_TO_DT[QUANT[qname]]
    out_f = 320
    r = rng(in_f, x_off, dt, 3)
    x, _ = fused_inputs(r, in_f)
    o = x_off // 4
    W = matrix(r, qname, out_f, in_f)
    h = r.standard_normal(out_f).astype(np.float32)
    ref = h + O.gemv(W, x[o:o + in_f], out_f, in_f, dt)
    Wd, xd, hd = on_device(W), DB.from_numpy(x), DB.from_numpy(h)
    ops.gemv_fused([(Wd, hd, out_f, dt)], xd.at(x_off), in_f, resid=hd)
    ops.synchronize()
    y = hd.numpy()
    assert np.isfinite(y).all() and not np.array_equal(y, h)
    err = float(np.abs(y - ref).max())
    print("resid %s in=%d x_off=%d: max err %.3g, bound %.3g" % (qname, in_f, x_off, err, tol_for(ref, in_f)))
    assert err <= tol_for(ref, in_f), err


@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("x_off", [0, 4])
@pytest.mark.parametrize("inter", [77, 864])
@pytest.mark.parametrize("in_f", FUSED_WIDTHS)
def test_gemv_fused_norm_gate_up_silu(qname, in_f, inter, x_off):
    """RMSNorm + gate | up + SiLU(gate) x up as one launch within 4 tol_for"""
    dt = G.GGML_TO_DT[QUANT[qname]]
    r = rng(in_f, inter, x_off, dt, 4)
    x, nw = fused_inputs(r, in_f)
    x /= 3
    o = x_off // 4
    Wg, Wu = matrix(r, qname, inter, in_f), matrix(r, qname, inter, in_f)
    xn = O.rmsnorm(x[o:o + in_f], nw[o:o + in_f], 1e-5).reshape(-1)
    ref = O.silu_mul(O.gemv(Wg, xn, inter, in_f, dt), O.gemv(Wu, xn, inter, in_f, dt))
    xd, nd, gd, ud = DB.from_numpy(x), DB.from_numpy(nw), on_device(Wg), on_device(Wu)
    od, scratch = DB.from_numpy(np.full(inter, np.nan, np.float32)), DB.zeros(inter * 4)
    ops.gemv_fused([(gd, od, inter, dt), (ud, scratch, inter, dt)], xd.at(x_off), in_f, norm_w=nd.at(x_off), eps=1e-5, silu_pair=True)
    ops.synchronize()
    y = od.numpy()
    assert np.isfinite(y).all()
    err = float(np.abs(y - ref).max())
    print("silu %s in=%d inter=%d x_off=%d: max err %.3g, bound %.3g" % (qname, in_f, inter, x_off, err, 4 * tol_for(ref, in_f)))
    assert err <= 4 * tol_for(ref, in_f), err


# ------------------------------------------------------------------------------- (3) what lies beside the operands takes no part
@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("form", ["gemv", "fused_norm"])
@pytest.mark.parametrize("in_f", [32, 96, 4064, 4128])
def test_bytes_beside_the_operands_take_no_part(qname, in_f, form):
    """W behind 32 guard bytes and in front of 64, x and the norm weights followed by 16 guard floats; once with guards of zeros, once with all-ones
    bytes (a NaN as a float, an FP16 NaN as a block scale).  The kernel may READ beside its operands inside the allocations (whole 16-byte
    chunks of a row, a float4 clamped to the row's end), but what it reads there must never reach a sum: the outputs of the two runs are the same
    bits, finite, and the oracle's within the form's bound."""
    dt = G.GGML_TO_DT[QUANT[qname]]
    out_f = 37
    r = rng(in_f, dt, 5)
    W = matrix(r, qname, out_f, in_f)
    x = r.standard_normal(in_f).astype(np.float32)
    nw = (1 + 0.05 * r.uniform(-1, 1, in_f)).astype(np.float32)
    outs = []
    for fill in (0x00, 0xFF):
        Wb = np.full(32 + W.nbytes + 64, fill, np.uint8)
        Wb[32:32 + W.nbytes] = W
        xb = np.full(4 * (in_f + 16), fill, np.uint8)
        xb[:4 * in_f] = x.view(np.uint8)
        nb = np.full(4 * (in_f + 16), fill, np.uint8)
        nb[:4 * in_f] = nw.view(np.uint8)
        Wd, xd, nd = DB.from_numpy(Wb), DB.from_numpy(xb), DB.from_numpy(nb)
        yd = DB.from_numpy(np.full(out_f, np.nan, np.float32))
        if form == "gemv":
            ops.launch_gemv(yd, Wd.at(32), xd, out_f, in_f, dt)
        else:
            ops.gemv_fused([(Wd.at(32), yd, out_f, dt)], xd, in_f, norm_w=nd, eps=1e-5)
        ops.synchronize()
        outs.append(yd.numpy(np.float32))
    assert np.isfinite(outs[0]).all() and np.isfinite(outs[1]).all()
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32))
    xin = x if form == "gemv" else O.rmsnorm(x, nw, 1e-5).reshape(-1)
    ref = O.gemv(W, xin, out_f, in_f, dt)
    assert np.abs(outs[1] - ref).max() <= (1 if form == "gemv" else 2) * tol_for(ref, in_f)


# ------------------------------------------------------------------------------- (5) contracts
def test_lane_major_form_is_refused_where_a_slice_is_not_whole_256_columns():
    """q8l_layout: no lane-major form for 320 / 864 / 4128 and for 11008 (3 x 3712) / 13824 (4 x 3456), themselves multiples of 256; one for 5120
    (2 x 2560) and 18944 (4 x 3840 + 3584).  The engine keeps the refused matrices as GGUF blocks (Model::repack_one)."""
    L = _lib.lib()
    d = DB.zeros(1 << 16)
    for in_f in (320, 864, 4128, 11008, 13824):
        assert ops.q8l_bytes(4, in_f) == 0, in_f
        assert L.ntk_q8l_pack(d.ptr, d.ptr, 4, in_f, None) == NTK_E_SHAPE, in_f
    for in_f in (5120, 18944):
        assert ops.q8l_bytes(4, in_f) == 4 * (in_f // 32 * 34), in_f


def test_lane_major_launch_over_320_columns_is_not_taken_and_writes_nothing():
    r = rng(320, 6)
    W = on_device(matrix(r, "Q8_0", 16, 320))
    x = DB.from_numpy(r.standard_normal(320).astype(np.float32))
    ys = [DB.from_numpy(np.full(n, np.nan, np.float32)) for n in (8, 4, 4)]
    segs = (_lib.GemvSeg * 3)()
    for i, (row0, n) in enumerate(((0, 8), (8, 4), (12, 4))):
        segs[i].W, segs[i].y, segs[i].rows, segs[i].dtype = W.at(row0 * 340), ys[i].ptr, n, G.DT_Q8_0
    assert _lib.lib().ntk_gemv_rp_fused(segs, 3, x.ptr, 320, None, 0.0, None, 0, None) in NOT_TAKEN
    ops.synchronize()
    assert all(np.isnan(y.numpy(np.float32)).all() for y in ys)


@pytest.mark.parametrize("qname", sorted(QUANT))
@pytest.mark.parametrize("in_f", [48, 32800])
def test_gemv_refuses_widths_it_cannot_serve_and_writes_nothing(qname, in_f):
    """48 columns: not whole blocks; 32800: nine slices (gemv_slices takes eight)"""
    dt = G.GGML_TO_DT[QUANT[qname]]
    Wd, xd = DB.zeros(4 * (in_f // 32 + 1) * 34 + 64), DB.zeros(4 * in_f)
    yd = DB.from_numpy(np.full(4, np.nan, np.float32))
    assert _lib.lib().ntk_gemv(yd.ptr, Wd.ptr, xd.ptr, 4, in_f, dt, None) == NTK_E_SHAPE
    ops.synchronize()
    assert np.isnan(yd.numpy(np.float32)).all()
