"""The three-piece bfloat16 split of an F32 activation, restated in numpy: what split_x_bf16_kernel of csrc/gemm_dense16.hip writes into its operand planes.

    p1 = rn(x), p2 = rn(x - p1), p3 = rn(x - p1 - p2)

rn rounds an F32 to the nearest bfloat16, ties to even, on the bit pattern (normals and subnormals alike); a FINITE value that would round to infinity keeps
the largest finite bfloat16 instead, and its remainder goes to the next piece like any other.  Inf and NaN stay what they are.  Both differences are exact in
F32: x - p1 has at most 16 significant bits, x - p1 - p2 at most 8."""
import numpy as np


def rn_bf16(x):
    """F32 array -> the nearest bfloat16 of every element, as F32 (low 16 bits zero)"""
    u = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    r = np.where((r & 0x7F80) == 0x7F80, r - 1, r)                         # a finite value never becomes infinite
    special = (u & 0x7F800000) == 0x7F800000
    r = np.where(special, (u >> 16) | np.where((u & 0x007FFFFF) != 0, np.uint64(0x40), np.uint64(0)), r)
    return (r.astype(np.uint32) << np.uint32(16)).view(np.float32)


def split3(x):
    """(p1, p2, p3) as F32 arrays"""
    x = np.ascontiguousarray(x, np.float32)
    with np.errstate(invalid="ignore"):
        p1 = rn_bf16(x)
        r1 = (x - p1).astype(np.float32)
        p2 = rn_bf16(r1)
        r2 = (r1 - p2).astype(np.float32)
        p3 = rn_bf16(r2)
    return p1, p2, p3
