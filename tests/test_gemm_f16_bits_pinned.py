"""GPU test: the prompt GEMM (csrc/gemm_f16.hip, gemm_f16_plan.h) gives the BITS recorded in tests/golden/gemm_f16_bits.json.

The other GEMM tests hold the three kernel forms to the oracle within a tolerance and to each other where the sums run in the same order: a changed
launch plan (another slice count, another tile height) or a changed summation order would pass most of them.  Here every form of the launch is pinned
to the output bytes of the commit the golden file was recorded from (tools/record_gemm_bits.py, which takes CASES and run_case from this module: the
two cannot disagree).  The file holds one SHA-256 per case over the bytes of all output buffers of the call; every buffer starts as NaN, or as the
residual (the row maxima that ntk_reduce_silu_mul_rowmax accumulates into: as zeros, which is what that call requires).

Cases -- the smallest shapes that reach each branch of the launch plan (csrc/gemm_f16_plan.h; tests/test_gemm_plan_cpu.py asserts with the plan
program that these shapes do reach them):
  formats   Q8_0, Q4_0, Q4_K, Q5_K, Q6_K over GGUF blocks and Q4_K, Q5_K, Q6_K over the decode repack (ops.rp_pack), each in every form it can take
  K-slice   one slice (T 5, in 512), several (in 1024: 2, in 4096: 8), one and two token blocks (T <= 16 / 17 .. 32), 32-row tiles (36864 rows)
  small     in 768 / 256 / 384 (no whole slices), one and two token blocks; Q6_K beyond 16 tokens; rows not on dword boundaries (Q6_K in 768)
  chunk     T 70 (a partial second chunk), 200 (K split in 4 or 2), 1024 x 4096 rows (32-row tiles; two chunks per workgroup where the format has
            that form), 1100 (two passes), rows not on dword boundaries (Q6_K in 256)
  fusions   three matrices sharing X in each form, the residual in place (with and without a K split), the K splits summed by
            ntk_reduce_rmsnorm_rowmax and ntk_reduce_silu_mul_rowmax, row maxima from the producer of X, planes written by prepare_x (reuse_x),
            full_form = 1 at 5 and 70 tokens (the same rows as the 1024-token call they are cut from)

Run on the MI355X box:  python -m pytest tests/test_gemm_f16_bits_pinned.py -m gpu -x -q
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

GOLDEN_FILE = os.path.join(GOLDEN, "gemm_f16_bits.json")
QUANT = {"Q8_0": G.GGML_Q8_0, "Q4_0": G.GGML_Q4_0, "Q4_K": G.GGML_Q4_K, "Q5_K": G.GGML_Q5_K, "Q6_K": G.GGML_Q6_K}
FORMATS = ["Q8_0", "Q4_0", "Q4_K", "Q5_K", "Q6_K", "Q4_K_RP", "Q5_K_RP", "Q6_K_RP"]
PASS = 1024        # tokens of one launch


def _case(fmt, T, in_f, rows, kind="plain"):
    rows = (rows,) if isinstance(rows, int) else tuple(rows)
    return dict(fmt=fmt, T=T, in_f=in_f, rows=rows, kind=kind, id="%s-t%d-i%d-r%s-%s" % (fmt, T, in_f, "+".join(str(r) for r in rows), kind))


def _cases():
    out = []
    for fmt in FORMATS:
        out += [_case(fmt, 5, 512, 64), _case(fmt, 20, 1024, 64),                   # K-slice: one slice; two slices, two token blocks (Q6_K: small)
                _case(fmt, 16, 4096, (512, 128, 128)), _case(fmt, 20, 4096, (512, 128, 128)),   # three matrices, 8 slices (Q6_K beyond 16 tokens: small)
                _case(fmt, 9, 768, 32), _case(fmt, 20, 256, 32),                    # small: three units over three waves; one unit (Q8_0 / Q4_0 at 20 tokens: chunk)
                _case(fmt, 70, 1024, 48), _case(fmt, 200, 1024, 256),               # chunk: 16-row tiles, K split
                _case(fmt, 70, 1024, (64, 32, 32)),                                 # ... three matrices
                _case(fmt, 1024, 512, 4096)]                                        # ... 32-row tiles; Q8_0: two chunks per workgroup, K split in two
    out += [_case("Q8_0", 5, 384, 64), _case("Q8_0", 9, 768, (64, 32, 32))]         # small: Q8_0's three units of 128 columns; three matrices
    out += [_case(fmt, 1024, 1024, 4096) for fmt in ("Q4_0", "Q4_K", "Q4_K_RP")]   # two chunks per workgroup of the 4-bit formats
    out += [_case(fmt, 5, 512, 36864) for fmt in ("Q8_0", "Q4_K_RP", "Q6_K")]      # K-slice, more 16-row tiles than one round of workgroups: 32-row tiles; Q6_K: two row groups per workgroup
    out += [_case(fmt, 1100, 256, 32) for fmt in ("Q8_0", "Q6_K")]                 # two passes; Q6_K: rows not on dword boundaries
    for fmt in ("Q8_0", "Q4_K"):
        out += [_case(fmt, T, i, r, "resid") for T, i, r in ((5, 512, 64), (16, 4096, 512), (9, 768, 32), (70, 1024, 48), (70, 256, 48))]
        out += [_case(fmt, T, i, r, "norm") for T, i, r in ((16, 4096, 512), (200, 1024, 256), (70, 256, 48))]
        out += [_case(fmt, T, i, (r, r), "silu") for T, i, r in ((20, 1024, 64), (70, 1024, 48), (70, 256, 48))]
        out += [_case(fmt, T, i, r, "rowmax") for T, i, r in ((5, 512, 64), (70, 1024, 48))]
        out += [_case(fmt, T, i, r, "prepared") for T, i, r in ((20, 1024, 64), (200, 1024, 256))]
        out += [_case(fmt, PASS, 512, 64, "full")]
    return out


CASES = _cases()
assert len({c["id"] for c in CASES}) == len(CASES)


def passes(c):
    """[(tokens, full_form)] of the launches case c makes"""
    if c["kind"] == "full":
        return [(PASS, 0), (5, 1), (70, 1)]
    return [(min(PASS, c["T"] - t0), 0) for t0 in range(0, c["T"], PASS)]


def rng(case_id):
    return np.random.Generator(np.random.Philox(key=[20261020, zlib.crc32(case_id.encode())]))


def _nan(n):
    return DB.from_numpy(np.full(n, np.nan, np.float32))


def run_case(c):
    """the call(s) of case c on fresh inputs -> its output buffers, one array each"""
    r = rng(c["id"])
    fmt, T, in_f, rows, kind = c["fmt"], c["T"], c["in_f"], c["rows"], c["kind"]
    rp = fmt.endswith("_RP")
    gt = QUANT[fmt[:4]]
    dt = G.GGML_TO_DT[gt]
    x = r.standard_normal((T, in_f)).astype(np.float32)
    x[:, in_f // 3] *= 50.0
    x[T // 2] *= 1e-3                                  # (tokens of different scales)
    X = DB.from_numpy(x)
    keep, W = [], []
    for n in rows:
        raw = DB.from_numpy(np.frombuffer(G.synth_tensor(r, gt, n, in_f), np.uint8))
        W.append(ops.rp_pack(raw, n, in_f, dt) if rp else raw)
        keep.append(raw)
    if kind in ("plain", "resid", "prepared", "rowmax"):
        res = r.standard_normal(T * rows[0]).astype(np.float32)
        Y = [DB.from_numpy(res) if kind == "resid" else _nan(T * n) for n in rows]
        segs = [(w, y, n, dt) for w, y, n in zip(W, Y, rows)]
        if kind == "prepared":
            ws = ops.gemm_workspace(in_f, sum(rows))
            assert ops.prepare_x("x", ws, T, in_f, X=X) == 0
            st = ops._gemm_quant_f16(segs, X, T, in_f, workspace=ws, reuse_x=1)
        elif kind == "rowmax":                         # X and its row maxima from the producer: the RMSNorm of x
            nw = DB.from_numpy((1.0 + 0.1 * r.standard_normal(in_f)).astype(np.float32))
            Xn, rm = _nan(T * in_f), _nan(T)
            ops.launch_rmsnorm_rowmax(Xn, X, nw, T, in_f, 1e-5, rm)
            st = ops.gemm_quant_ws_rm(Y[0], W[0], Xn, T, rows[0], in_f, dt, rm)
        else:
            st = ops._gemm_quant_f16(segs, X, T, in_f, resid=Y[0] if kind == "resid" else None, repacked=rp)
        assert st == 0, st
        ops.synchronize()
        return [y.numpy(np.float32)[:T * n].copy() for y, n in zip(Y, rows)]
    if kind == "norm":                                 # Wo / down + residual + the next RMSNorm: the K splits summed by the consumer
        H = rows[0]
        hidden = DB.from_numpy(r.standard_normal(T * H).astype(np.float32))
        nw = DB.from_numpy((1.0 + 0.1 * r.standard_normal(H)).astype(np.float32))
        x_out, rm = _nan(T * H), _nan(T)
        ops.gemm_deferred_then_consumer("norm", W[0], X, T, H, in_f, dt, hidden=hidden, weight=nw, eps=1e-5, x_out=x_out, row_max_out=rm)
        return [hidden.numpy(np.float32)[:T * H].copy(), x_out.numpy(np.float32)[:T * H].copy(), rm.numpy(np.float32)[:T].copy()]
    if kind == "silu":                                 # gate | up + SiLU x up
        I = rows[0]
        out, rm = _nan(T * I), DB.from_numpy(np.zeros(T, np.float32))
        ops.gemm_deferred_then_consumer("silu", (W[0], W[1]), X, T, I, in_f, dt, output=out, row_max_out=rm)
        return [out.numpy(np.float32)[:T * I].copy(), rm.numpy(np.float32)[:T].copy()]
    assert kind == "full"                              # the whole pass, then its first 5 and 70 tokens alone with full_form = 1
    outs = []
    for t, full in passes(c):
        y = _nan(t * rows[0])
        assert ops._gemm_quant_f16([(W[0], y, rows[0], dt)], X, t, in_f, full_form=bool(full), repacked=rp) == 0
        outs.append(y.numpy(np.float32)[:t * rows[0]].copy())
    return outs


def digest(outs):
    h = hashlib.sha256()
    for y in outs:
        h.update(np.ascontiguousarray(y).view(np.uint8).tobytes())
    return h.hexdigest()


def check(c, outs):
    """what must hold of a case's outputs whatever was recorded"""
    assert all(np.isfinite(y).all() for y in outs), c["id"]
    if c["kind"] == "full":
        whole, n = outs[0], c["rows"][0]
        for y in outs[1:]:
            assert np.array_equal(y.view(np.uint32), whole[:y.size].view(np.uint32)), "%s: %d tokens with full_form" % (c["id"], y.size // n)


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
    check(c, outs)
    assert digest(outs) == golden[c["id"]]
