"""GPU test: the decode GEMV (csrc/gemv.hip, gemv_core.hip.h) gives the BITS recorded in tests/golden/gemv_bits.json.

The other GEMV tests pin the lane-major kernel to the kernel over GGUF blocks bit for bit, and that one to the oracle within a tolerance: a changed
summation order in the raw forms would pass them.  Here every form of the launch is pinned to the output bytes of the commit the golden file was
recorded from (tools/record_gemv_bits.py, which takes CASES and run_case from this module: the two cannot disagree).  The file holds one
SHA-256 per case over the bytes of all output buffers of the call; every buffer starts as NaN, or as the residual.

Cases -- the smallest shapes at which each piece of the kernel can go wrong:
  formats   Q8_0, Q4_0, Q4_K, Q5_K, Q6_K over GGUF blocks (ops.gemv_fused); Q8L = Q8_0 lane-major (ops.q8l_pack + ops.gemv_rp_fused)
  widths    256 (one K-quant block, 4 live lanes), 288 (a lane with 32 of its 64 columns), 4096 (a full slice), 4608 (two slices of 2304: the
            smallest multi-slice width of every format that still takes the fast prologue), 12288 (three slices, 6-wave workgroups),
            14336 (four slices of 56 live lanes), 28672 (seven slices, the image in two passes, LDS above 64 KiB; with the norm: plain prologue)
  rows      1, 7 (most waves without a row, a partial batch), 4100 (a second row per wave: the prefetch, both register sets), 8200 at the
            multi-slice widths (a full batch of 4, then a partial one: both halves of the partial-sum buffer)
  fusions   plain, norm, residual in place, silu_pair, three unequal segments sharing x (the cursor crosses segments), norm + three segments
  forms     integer activations (Q4_K / Q6_K), two formats in one launch (Q4_K + Q6_K / Q5_K), W offset by 2 bytes (the general decoders,
            delta != 0), x offset by 4 bytes (the plain prologue)

Run on the MI355X box:  python -m pytest tests/test_gemv_bits_pinned.py -m gpu -x -q
"""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

from conftest import GOLDEN
from ntransformer_amd import gguf as G
from ntransformer_amd import ops
from ntransformer_amd.ops import DeviceBuffer as DB

pytestmark = pytest.mark.gpu

GOLDEN_FILE = os.path.join(GOLDEN, "gemv_bits.json")
QUANT = {"Q8_0": G.GGML_Q8_0, "Q4_0": G.GGML_Q4_0, "Q4_K": G.GGML_Q4_K, "Q5_K": G.GGML_Q5_K, "Q6_K": G.GGML_Q6_K, "Q8L": G.GGML_Q8_0}
FUSIONS = ["plain", "norm", "resid", "silu", "seg3", "norm_seg3"]
MULTI = (4608, 12288, 14336)     # the multi-slice widths that get 8200 rows


def _widths(fmt):
    if fmt in ("Q4_K", "Q5_K", "Q6_K"):
        return [256, 4096, 4608, 14336]
    w = [256, 288, 4096, 4608, 12288, 14336, 28672]
    return [v for v in w if v != 288] if fmt == "Q8L" else w      # (the lane-major layout needs slices of whole 256 columns)


def _case(fmt, in_f, rows, fusion, **kw):
    c = dict(fmt=fmt, in_f=in_f, rows=rows, fusion=fusion, xi=False, w_off=0, x_off=0, other=None)
    c.update(kw)
    name = "%s-%d-r%d-%s" % (fmt, in_f, rows, fusion)
    if c["xi"]: name += "-xi"
    if c["w_off"]: name += "-w%d" % c["w_off"]
    if c["x_off"]: name += "-x%d" % c["x_off"]
    if c["other"]: name += "-" + c["other"]
    c["id"] = name
    return c


def _cases():
    out = []
    for fmt in QUANT:
        for in_f in _widths(fmt):
            if in_f == 28672:
                rows_fus = [(r, f) for r in (7, 520) for f in FUSIONS]
            else:
                rows_fus = [(1, "plain")] + [(7, f) for f in FUSIONS]
                if in_f in MULTI:      # (8200 rows carry every fusion: 4100 keep one of each kind of epilogue)
                    rows_fus += [(4100, f) for f in ("plain", "silu", "norm_seg3")] + [(8200, f) for f in FUSIONS]
                else:
                    rows_fus += [(4100, f) for f in FUSIONS]
            out += [_case(fmt, in_f, r, f) for r, f in rows_fus]
    for fmt in ("Q4_K", "Q6_K"):             # the integer-activation form
        for in_f in (4096, 4608):
            out += [_case(fmt, in_f, r, f, xi=True) for r in (7, 4100) for f in ("plain", "norm", "resid", "silu", "norm_seg3")]
    for other in ("Q6_K", "Q5_K"):           # two formats in one launch: segments 0, 1 Q4_K, segment 2 `other`
        out += [_case("Q4_K", 4096, r, f, other=other) for r in (7, 4100) for f in ("seg3", "norm_seg3")]
    for fmt in ("Q8_0", "Q4_0", "Q4_K", "Q5_K", "Q6_K"):      # W offset by 2 bytes
        for in_f in (4096, 4608):
            out += [_case(fmt, in_f, r, f, w_off=2) for r, f in ((7, "norm_seg3"), (4100, "plain"), (4100, "silu"))]
    for fmt in ("Q8_0", "Q4_0", "Q4_K", "Q5_K", "Q6_K"):      # x offset by 4 bytes (the call over lane-major rows refuses such an x)
        for in_f in (4096, 4608):
            out += [_case(fmt, in_f, r, f, x_off=4) for r, f in ((7, "norm_seg3"), (4100, "plain"), (4100, "norm"))]
    return out


CASES = _cases()
assert len({c["id"] for c in CASES}) == len(CASES)


def rng(case_id):
    return np.random.Generator(np.random.Philox(key=[20261019, zlib.crc32(case_id.encode())]))


def segments(c):
    """[(first row, rows)] of the call: silu_pair -- gate and up of rows / 2 rows each from 4100 rows on (a wave then walks as many items as in
    the plain case); three segments -- unequal, none empty from 7 rows on"""
    n, f = c["rows"], c["fusion"]
    if f == "silu":
        h = n // 2 if n >= 4100 else n
        return [(0, h), (h, h)]
    if f in ("seg3", "norm_seg3"):
        a, b = n // 2 + 1, n // 3
        return [(0, a), (a, b), (a + b, n - a - b)]
    return [(0, n)]


def run_case(c):
    """the call of case c on fresh inputs -> the bytes of its output buffers, one array per segment"""
    r = rng(c["id"])
    fmt, in_f, f = c["fmt"], c["in_f"], c["fusion"]
    segs = segments(c)
    gts = [QUANT[fmt]] * len(segs)
    if c["other"]: gts[2] = QUANT[c["other"]]
    x = r.standard_normal(in_f + 1).astype(np.float32)
    x[1 + in_f // 3] *= 50.0
    nw = (1.0 + 0.1 * r.standard_normal(in_f + 1)).astype(np.float32)
    res = r.standard_normal(segs[0][1]).astype(np.float32)
    norm, resid = f in ("norm", "norm_seg3"), f == "resid"
    xo = c["x_off"] // 4             # x and the norm weights start x_off bytes into their (16-byte aligned) allocations
    xd, nwd = DB.from_numpy(x), DB.from_numpy(nw)
    keep, call = [], []
    for i, ((r0, n), gt) in enumerate(zip(segs, gts)):
        raw = np.frombuffer(G.synth_tensor(r, gt, n, in_f), np.uint8)
        Wd = DB(raw.nbytes + c["w_off"] + 64)
        Wd.upload(raw, c["w_off"])
        W = Wd.at(c["w_off"])
        if fmt == "Q8L":
            keep.append(Wd)
            Wd = ops.q8l_pack(Wd, n, in_f)
            W = Wd.ptr
        y = DB.from_numpy(res if resid and i == 0 else np.full(n, np.nan, np.float32))
        keep += [Wd, y]
        call.append((W, y, n, G.GGML_TO_DT[gt]))
    kw = dict(norm_w=nwd.at(4 * xo) if norm else None, eps=1e-5 if norm else 0.0, resid=call[0][1] if resid else None, silu_pair=f == "silu")
    if fmt == "Q8L":
        ops.gemv_rp_fused(call, xd.at(4 * xo), in_f, **kw)
    else:
        ops.gemv_fused(call, xd.at(4 * xo), in_f, integer_activations=True if c["xi"] else None, **kw)
    ops.synchronize()
    return [y.numpy(np.float32)[:n].copy() for (_, y, n, _) in call]


def digest(outs):
    h = hashlib.sha256()
    for y in outs:
        h.update(np.ascontiguousarray(y).view(np.uint8).tobytes())
    return h.hexdigest()


def written(c, outs):
    """the buffers the call stores to (silu_pair: the first one only)"""
    return outs[:1] if c["fusion"] == "silu" else outs


@pytest.fixture(scope="module", autouse=True)
def _device():
    ops.init(0)
    yield
    ops.synchronize()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN_FILE) as f:
        return json.load(f)["cases"]


@pytest.mark.parametrize("c", CASES, ids=[c["id"] for c in CASES])
def test_output_bits_are_the_recorded_ones(c, golden):
    outs = run_case(c)
    assert all(np.isfinite(y).all() for y in written(c, outs))
    assert digest(outs) == golden[c["id"]]
