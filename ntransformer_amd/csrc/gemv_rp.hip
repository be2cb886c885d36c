// gemv_rp.hip -- K-quant decode GEMV on the int8 matrix cores, from an ENGINE-OWNED load-time repack of the GGUF blocks
// (SURVEY 7.1 step 7 / 8(b) "Ownership": repack buffers belong to the engine; the 1:1 ntk_gemv keeps taking raw GGUF).
//
// Replaces, for the engine's fused decode path, gemv_q4_k / q5_k / q6_k_kernel of the reference (src/cuda/gemm.cu:158-470):
// the same weights (bit-identical integers and scales, checked by ntk_rp_dequant), the same factorisation
//      y[r] = sum_sb  d * ( sum_j sc_j * sum_{k in j} q_k x_k )  -  dmin * sum_j m_j * sum_{k in j} x_k          (Q4_K / Q5_K)
//      y[r] = sum_sb  d * ( sum_j sc_j * sum_{k in j} q_k x_k )  -  32 d * sum_j sc_j * sum_{k in j} x_k          (Q6_K)
// with the inner sums as EXACT integer dot products: x is converted once per workgroup into three signed base-256 digit planes
// X_k = rint(x_k 2^(22-e)) (e = exponent of the largest |x| of the 256-column super-block; error per term <= half a unit, at most 2^-22 of that maximum,
// the level of the F32 rounding it replaces), and v_mfma_i32_16x16x64_i8 multiplies 16 weight rows x 64 columns by the digit
// planes of the two (four) sub-blocks the 64 columns span.  Why: the VALU decoders of gemv.hip issue ~250 vector instructions per
// 4096 weights and are bound by that (84 % VALU issue, 0.51-0.67 of HBM on the long launches, profiles/r03_gemv_microbench.txt);
// here the unpack is 3 instructions per 8 weights, the per-(row, sub-block) scale work 4 per 1024 weights, and nothing is staged
// through LDS: a wave's 1 KiB load IS the B operand of two MFMAs.
//
// Repacked layout ("rp", one allocation per tensor; tile = 16 rows, item = tile x 256-column super-block):
//   P1 [tile][sb][step 0..1][S1 bytes]   step = 128 columns.  Bytes 16 l .. 16 l + 15 belong to lane l = 16 kg + i (row i of the tile):
//        byte b: low nibble  = low 4 bits of the quant of column 128 s + 16 kg + b        (operand of the MFMA of half 0)
//                high nibble = ...                          column 128 s + 64 + 16 kg + b   (half 1)
//        Q5_K: + 256 bytes, dword l: bit 8 y + 4 h + v = bit 4 of the quant of column 128 s + 64 h + 16 kg + 4 v + y
//        Q6_K: + 512 bytes, dwords 2 l + h: bits 8 y + 2 v (+1) = bits 4..5 of the quant of that column
//   P2 [tile][sb][S2 bytes]   16 rows x 16 bytes: Q4_K / Q5_K {sc[8], m[8]} (the 6-bit values as bytes), Q6_K sc[16] (int8);
//        then 16 x {d, dmin} (FP16 pairs; Q6_K: 16 x d).
//   Bytes: Q4_K 2368 per item (GGUF 2304: 1.028 x), Q5_K 2880 (2816: 1.023 x), Q6_K 3360 (3360: 1.000 x).
//   Rows are padded to whole tiles with zero weights.
//
// MFMA roles: first operand (M = 16) = digit planes of x from LDS, entry m = 4 jj + p (sub-block jj of the 64 columns, digit p; p = 3
// unused), zero outside its own sub-block; second operand (N = 16) = the 16 weight rows.  Accumulator lane (row i = lane & 15,
// mg = lane >> 4) register r = digit r of sub-block mg: a lane scales ITS row by ITS sub-block's scale (v_bfe + 3 v_mad_i32_i24),
// sums the super-block in integers, and converts once per super-block.  The minimum / offset term is one more MFMA per super-block:
// the row's m[8] (sc[16]) against the digits of the sub-block sums of X.
#include "common.hip.h"
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace ntk {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef uint32_t u4 __attribute__((ext_vector_type(4)));
typedef uint32_t u2 __attribute__((ext_vector_type(2)));

template <int DT> struct Rp;
template <> struct Rp<NTK_DT_Q4_K> { static constexpr int S1 = 1024, S2 = 320, BB = 144, NSUB = 8; };
template <> struct Rp<NTK_DT_Q5_K> { static constexpr int S1 = 1280, S2 = 320, BB = 176, NSUB = 8; };
template <> struct Rp<NTK_DT_Q6_K> { static constexpr int S1 = 1536, S2 = 288, BB = 210, NSUB = 16; };

static bool rp_supported(int dt) { return dt == NTK_DT_Q4_K || dt == NTK_DT_Q5_K || dt == NTK_DT_Q6_K; }
static size_t rp_s1(int dt) { return dt == NTK_DT_Q4_K ? 1024 : dt == NTK_DT_Q5_K ? 1280 : 1536; }
static size_t rp_s2(int dt) { return dt == NTK_DT_Q6_K ? 288 : 320; }

// ------------------------------------------------------------------------------------------------------------------
// raw GGUF accessors (reference src/core/types.h:112-137): the quant integer of column cc of a super-block
// ------------------------------------------------------------------------------------------------------------------
template <int DT> __device__ __forceinline__ int raw_q(const uint8_t* blk, int cc) {
    if constexpr (DT == NTK_DT_Q4_K || DT == NTK_DT_Q5_K) {
        const int chunk = cc >> 6, l = cc & 31, hi = (cc >> 5) & 1;
        const uint8_t* qs = blk + (DT == NTK_DT_Q4_K ? 16 : 48);
        const int by = qs[32 * chunk + l];
        int q = hi ? (by >> 4) : (by & 15);
        if constexpr (DT == NTK_DT_Q5_K) q |= ((blk[16 + l] >> (2 * chunk + hi)) & 1) << 4;
        return q;
    } else {
        const int n = cc >> 7, quarter = (cc >> 5) & 3, l = cc & 31;
        const int by = blk[64 * n + l + ((quarter & 1) ? 32 : 0)];
        const int nib = (quarter >= 2) ? (by >> 4) : (by & 15);
        const int hi2 = (blk[128 + 32 * n + l] >> (2 * quarter)) & 3;
        return nib | (hi2 << 4);
    }
}

// P1 + P2 of one item (tile, sb): 128 threads build the two step records, 16 the row records
template <int DT>
__global__ __launch_bounds__(128) void rp_pack_kernel(uint8_t* __restrict__ dst, const uint8_t* __restrict__ raw, int rows, int nsb, size_t p2_off) {
    using F = Rp<DT>;
    const int item = blockIdx.x, tile = item / nsb, sb = item - tile * nsb;
    const int t = threadIdx.x, s = t >> 6, l = t & 63, i = l & 15, kg = l >> 4;
    const int row = 16 * tile + i;
    const bool live = row < rows;
    const size_t row_bytes = (size_t)nsb * F::BB;
    const uint8_t* blk = raw + (size_t)(live ? row : 0) * row_bytes + (size_t)sb * F::BB;
    uint8_t* p1 = dst + (size_t)item * (2 * F::S1) + (size_t)s * F::S1;
    uint32_t w[4] = {0u, 0u, 0u, 0u}, hb = 0u, hh[2] = {0u, 0u};
    if (live) {
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            const int c0 = 128 * s + 16 * kg + b;
            const int q0 = raw_q<DT>(blk, c0), q1 = raw_q<DT>(blk, c0 + 64);
            w[b >> 2] |= (uint32_t)((q0 & 15) | ((q1 & 15) << 4)) << (8 * (b & 3));
            const int v = b >> 2, y = b & 3;
            if constexpr (DT == NTK_DT_Q5_K) hb |= (uint32_t)((q0 >> 4) & 1) << (8 * y + v) | (uint32_t)((q1 >> 4) & 1) << (8 * y + 4 + v);
            if constexpr (DT == NTK_DT_Q6_K) { hh[0] |= (uint32_t)((q0 >> 4) & 3) << (8 * y + 2 * v); hh[1] |= (uint32_t)((q1 >> 4) & 3) << (8 * y + 2 * v); }
        }
    }
    *reinterpret_cast<u4*>(p1 + 16 * l) = u4{w[0], w[1], w[2], w[3]};
    if constexpr (DT == NTK_DT_Q5_K) *reinterpret_cast<uint32_t*>(p1 + 1024 + 4 * l) = hb;
    if constexpr (DT == NTK_DT_Q6_K) *reinterpret_cast<u2*>(p1 + 1024 + 8 * l) = u2{hh[0], hh[1]};
    if (t < 16) {   // row record of row t
        const int r = 16 * tile + t;
        const bool lv = r < rows;
        const uint8_t* b2 = raw + (size_t)(lv ? r : 0) * row_bytes + (size_t)sb * F::BB;
        uint8_t* p2 = dst + p2_off + (size_t)item * F::S2;
        uint8_t rec[16];
        uint16_t d = 0, dmin = 0;
        for (int k = 0; k < 16; ++k) rec[k] = 0;
        if (lv) {
            if constexpr (DT == NTK_DT_Q6_K) {
                for (int k = 0; k < 16; ++k) rec[k] = b2[192 + k];
                d = (uint16_t)(b2[208] | (b2[209] << 8));
            } else {
                uint32_t s0, s1, s2;
                __builtin_memcpy(&s0, b2 + 4, 4); __builtin_memcpy(&s1, b2 + 8, 4); __builtin_memcpy(&s2, b2 + 12, 4);
                for (int j = 0; j < 8; ++j) {
                    float sc, mn;
                    kq_scale_min(s0, s1, s2, j, sc, mn);
                    rec[j] = (uint8_t)(int)sc; rec[8 + j] = (uint8_t)(int)mn;
                }
                d = (uint16_t)(b2[0] | (b2[1] << 8)); dmin = (uint16_t)(b2[2] | (b2[3] << 8));
            }
        }
        for (int k = 0; k < 16; ++k) p2[16 * t + k] = rec[k];
        if constexpr (DT == NTK_DT_Q6_K) *reinterpret_cast<uint16_t*>(p2 + 256 + 2 * t) = d;
        else *reinterpret_cast<uint32_t*>(p2 + 256 + 4 * t) = (uint32_t)d | ((uint32_t)dmin << 16);
    }
}

// ---- the raw GGUF blocks back from the repacked form (round 5: ONE resident copy of a K-quant matrix -- the engine frees the uploaded GGUF bytes
//      after the repack and, for the launches that read raw blocks (the prompt GEMM of gemm_f16.hip, the 1:1 ntk_gemv), unpacks the tensor into
//      a scratch right in front of them).  Exact inverse of rp_pack_kernel: the repack holds the same integers and the same 6-bit / int8 scales,
//      so the bytes come back as they were uploaded (tests/test_gemv_rp.py::test_unpack_restores_the_gguf_bytes).  One workgroup per item
//      (16 rows x one 256-column super-block): the item's planes into LDS, then every thread assembles output words. ----
template <int DT>
__device__ __forceinline__ int rp_q_lds(const uint8_t* p1, int i, int c) {   // quant of (row i, column c of the super-block), as rp_dequant_kernel
    using F = Rp<DT>;
    const int s = c >> 7, h = (c >> 6) & 1, kg = (c >> 4) & 3, b = c & 15, l = 16 * kg + i;
    const uint8_t* ps = p1 + (size_t)s * F::S1;
    const int by = ps[16 * l + b];
    int q = h ? (by >> 4) : (by & 15);
    const int v = b >> 2, y = b & 3;
    if constexpr (DT == NTK_DT_Q5_K) q |= (int)((*reinterpret_cast<const uint32_t*>(ps + 1024 + 4 * l) >> (8 * y + 4 * h + v)) & 1u) << 4;
    if constexpr (DT == NTK_DT_Q6_K) q |= (int)((*reinterpret_cast<const uint32_t*>(ps + 1024 + 8 * l + 4 * h) >> (8 * y + 2 * v)) & 3u) << 4;
    return q;
}
template <int DT>
__device__ __forceinline__ uint32_t rp_raw_byte(const uint8_t* p1, const uint8_t* p2, int i, int B) {   // byte B of row i's GGUF block
    if constexpr (DT == NTK_DT_Q6_K) {   // ql[128] qh[64] scales[16] d   (types.h:132-137)
        if (B < 128) {
            const int n = B >> 6, l = B & 31, odd = (B >> 5) & 1;              // ql[64 n + l + 32 odd]: q(128n + 32 odd + l) | q(128n + 64 + 32 odd + l) << 4
            const int c0 = 128 * n + 32 * odd + l;
            return (uint32_t)((rp_q_lds<DT>(p1, i, c0) & 15) | ((rp_q_lds<DT>(p1, i, c0 + 64) & 15) << 4));
        }
        if (B < 192) {
            const int n = (B - 128) >> 5, l = (B - 128) & 31;
            uint32_t v = 0;
#pragma unroll
            for (int quarter = 0; quarter < 4; ++quarter) v |= (uint32_t)(rp_q_lds<DT>(p1, i, 128 * n + 32 * quarter + l) >> 4) << (2 * quarter);
            return v;
        }
        if (B < 208) return p2[16 * i + (B - 192)];
        return p2[256 + 2 * i + (B - 208)];
    } else {                             // d dmin scales[12] (qh[32]) qs[128]   (types.h:112-128)
        constexpr int QS0 = DT == NTK_DT_Q5_K ? 48 : 16;
        if (B < 4) return p2[256 + 4 * i + B];
        if (B < 16) {                    // the 6-bit (scale, min) pairs, packed as gemm.cu:206-222 unpacks them
            const int j = (B - 4) & 3, grp = (B - 4) >> 2;
            const uint32_t sc_lo = p2[16 * i + j], sc_hi = p2[16 * i + 4 + j], mn_lo = p2[16 * i + 8 + j], mn_hi = p2[16 * i + 12 + j];
            if (grp == 0) return (sc_lo & 63u) | ((sc_hi >> 4) << 6);
            if (grp == 1) return (mn_lo & 63u) | ((mn_hi >> 4) << 6);
            return (sc_hi & 15u) | ((mn_hi & 15u) << 4);
        }
        if (DT == NTK_DT_Q5_K && B < 48) {
            const int l = B - 16;
            uint32_t v = 0;
#pragma unroll
            for (int k = 0; k < 8; ++k) v |= (uint32_t)((rp_q_lds<DT>(p1, i, 64 * (k >> 1) + 32 * (k & 1) + l) >> 4) & 1) << k;
            return v;
        }
        const int b = B - QS0, chunk = b >> 5, l = b & 31;
        return (uint32_t)((rp_q_lds<DT>(p1, i, 64 * chunk + l) & 15) | ((rp_q_lds<DT>(p1, i, 64 * chunk + 32 + l) & 15) << 4));
    }
}
// Word-wise: the repack pairs the columns (c, c + 64) of a 128-column step in one byte, Q6_K's ql pairs the same columns (a 16-byte chunk of a
// lane IS 16 bytes of the row's ql), Q4_K / Q5_K pair (c, c + 32): two masks and a shift per output dword; the fifth / sixth bits come out of the
// lanes' bit planes four bytes at a time.  The rows are assembled in LDS and written out in one coalesced pass (first form: a byte at a time
// through rp_raw_byte, 1 TB/s -- a 1024-token prompt pass of a 70B Q6_K model lost 11 % to it; this one: profiles/r05_repack_one_resident_copy.txt).
template <int DT>
__global__ __launch_bounds__(256) void rp_unpack_kernel(uint8_t* __restrict__ raw, const uint8_t* __restrict__ rp, int rows, int nsb, size_t p2_off) {
    using F = Rp<DT>;
    constexpr int PITCH = (F::BB + 15) & ~15;   // (16-byte row starts: the ql chunks go in as b128 stores)
    __shared__ __attribute__((aligned(16))) uint8_t img[2 * F::S1 + F::S2];
    __shared__ __attribute__((aligned(16))) uint8_t outb[16 * PITCH];
    const int item = blockIdx.x, tile = item / nsb, sb = item - tile * nsb, t = threadIdx.x;
    const uint8_t* g1 = rp + (size_t)item * (2 * F::S1);
    const uint8_t* g2 = rp + p2_off + (size_t)item * F::S2;
    for (int k = t; k < 2 * F::S1 / 16; k += 256) *reinterpret_cast<u4*>(img + 16 * k) = *reinterpret_cast<const u4*>(g1 + 16 * k);
    for (int k = t; k < F::S2 / 16; k += 256) *reinterpret_cast<u4*>(img + 2 * F::S1 + 16 * k) = *reinterpret_cast<const u4*>(g2 + 16 * k);
    __syncthreads();
    const uint8_t* p1 = img;
    const uint8_t* p2 = img + 2 * F::S1;
    const int i = t & 15;
    uint8_t* row = outb + i * PITCH;
    auto ld32 = [&](const uint8_t* p) { return *reinterpret_cast<const uint32_t*>(p); };
    if constexpr (DT == NTK_DT_Q6_K) {   // ql[128] qh[64] scales[16] d   (types.h:132-137)
        if (t < 128) {                   // ql[64 s + 16 kg ..]: the lane's 16-byte chunk of step s
            const int kg = (t >> 4) & 3, s = t >> 6;
            *reinterpret_cast<u4*>(row + 64 * s + 16 * kg) = *reinterpret_cast<const u4*>(p1 + (size_t)s * F::S1 + 16 * (16 * kg + i));
        }
        {                                // qh[32 s + 16 half + 4 w ..+3]: two bits of each of the four 32-column quarters
            const int w = (t >> 4) & 3, half = (t >> 6) & 1, s = t >> 7;
            const uint8_t* hp = p1 + (size_t)s * F::S1 + 1024;
            uint32_t v = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {   // quarter j: lanes kg = 2 (j & 1) + half, plane j >> 1 (columns c / c + 64)
                const uint32_t src = ld32(hp + 8 * (16 * (2 * (j & 1) + half) + i) + 4 * (j >> 1));
                v |= ((src >> (2 * w)) & 0x03030303u) << (2 * j);
            }
            *reinterpret_cast<uint32_t*>(row + 128 + 32 * s + 16 * half + 4 * w) = v;
        }
        if (t < 64) *reinterpret_cast<uint32_t*>(row + 192 + 4 * (t >> 4)) = ld32(p2 + 16 * i + 4 * (t >> 4));
        if (t < 16) *reinterpret_cast<uint16_t*>(row + 208) = *reinterpret_cast<const uint16_t*>(p2 + 256 + 2 * i);
    } else {                             // d dmin scales[12] (qh[32]) qs[128]   (types.h:112-128)
        constexpr int QS0 = DT == NTK_DT_Q5_K ? 48 : 16;
        {                                // qs[32 (2 s + h) + 4 g ..+3], h = 0 / 1: low / high nibbles of lanes kg = g >> 2 and 2 + (g >> 2)
            const int g = (t >> 4) & 7, s = t >> 7;
            const uint8_t* sp = p1 + (size_t)s * F::S1 + 4 * (g & 3);
            const uint32_t A = ld32(sp + 16 * (16 * (g >> 2) + i)), B = ld32(sp + 16 * (16 * (2 + (g >> 2)) + i));
            *reinterpret_cast<uint32_t*>(row + QS0 + 64 * s + 4 * g) = (A & 0x0F0F0F0Fu) | ((B & 0x0F0F0F0Fu) << 4);
            *reinterpret_cast<uint32_t*>(row + QS0 + 64 * s + 32 + 4 * g) = ((A >> 4) & 0x0F0F0F0Fu) | (B & 0xF0F0F0F0u);
        }
        if constexpr (DT == NTK_DT_Q5_K) {
            if (t < 128) {               // qh[4 g ..+3]: bit 2 (2 s + h) + hi of byte l' <- bit 8 y + 4 h + w of lane kg = 2 hi + (g >> 2), step s
                const int g = t >> 4, w = g & 3;
                uint32_t v = 0;
#pragma unroll
                for (int s = 0; s < 2; ++s)
#pragma unroll
                    for (int hi = 0; hi < 2; ++hi) {
                        const uint32_t H = ld32(p1 + (size_t)s * F::S1 + 1024 + 4 * (16 * (2 * hi + (g >> 2)) + i));
#pragma unroll
                        for (int h = 0; h < 2; ++h) v |= ((H >> (4 * h + w)) & 0x01010101u) << (2 * (2 * s + h) + hi);
                    }
                *reinterpret_cast<uint32_t*>(row + 16 + 4 * g) = v;
            }
        }
        if (t < 64) {                    // d, dmin and the 12 packed scale bytes (gemm.cu:206-222 unpacks them)
            const int u = t >> 4;
            uint32_t w = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) w |= rp_raw_byte<DT>(p1, p2, i, 4 * u + e) << (8 * e);
            *reinterpret_cast<uint32_t*>(row + 4 * u) = w;
        }
    }
    __syncthreads();
    constexpr int UB = DT == NTK_DT_Q6_K ? 2 : 4, U = F::BB / UB;   // Q6_K blocks are 210 bytes at 2-byte alignment: halfword stores
    for (int k = t; k < 16 * U; k += 256) {
        const int r = k / U, u = k - r * U, grow = 16 * tile + r;
        if (grow >= rows) continue;
        uint8_t* dst = raw + ((size_t)grow * nsb + sb) * F::BB + (size_t)UB * u;
        if constexpr (UB == 2) *reinterpret_cast<uint16_t*>(dst) = *reinterpret_cast<const uint16_t*>(outb + r * PITCH + 2 * u);
        else *reinterpret_cast<uint32_t*>(dst) = *reinterpret_cast<const uint32_t*>(outb + r * PITCH + 4 * u);
    }
}

// the weights back as floats from the repacked form, with the block formulas of SURVEY Appendix A evaluated product by product
// (no contraction): w = (d sc) q - (dmin m)   /   w = (d sc) (q - 32).  out [rows][in].  Test / parity instrumentation.
template <int DT>
__global__ __launch_bounds__(256) void rp_dequant_kernel(float* __restrict__ out, const uint8_t* __restrict__ rp, int rows, int in, int nsb, size_t p2_off) {
    using F = Rp<DT>;
    const int row = blockIdx.x;
    const int tile = row >> 4, i = row & 15;
    for (int col = threadIdx.x; col < in; col += blockDim.x) {
        const int sb = col >> 8, c = col & 255, s = c >> 7, h = (c >> 6) & 1, kg = (c >> 4) & 3, b = c & 15, l = 16 * kg + i;
        const size_t item = (size_t)tile * nsb + sb;
        const uint8_t* p1 = rp + item * (2 * F::S1) + (size_t)s * F::S1;
        const uint8_t* p2 = rp + p2_off + item * F::S2;
        const int by = p1[16 * l + b];
        int q = h ? (by >> 4) : (by & 15);
        const int v = b >> 2, y = b & 3;
        if constexpr (DT == NTK_DT_Q5_K) q |= (int)((*reinterpret_cast<const uint32_t*>(p1 + 1024 + 4 * l) >> (8 * y + 4 * h + v)) & 1u) << 4;
        if constexpr (DT == NTK_DT_Q6_K) q |= (int)((*reinterpret_cast<const uint32_t*>(p1 + 1024 + 8 * l + 4 * h) >> (8 * y + 2 * v)) & 3u) << 4;
        float w;
        if constexpr (DT == NTK_DT_Q6_K) {
            const float d = h2f(*reinterpret_cast<const uint16_t*>(p2 + 256 + 2 * i));
            const float sc = (float)(int)(int8_t)p2[16 * i + (c >> 4)];
            w = __fmul_rn(__fmul_rn(d, sc), (float)(q - 32));
        } else {
            const uint32_t dd = *reinterpret_cast<const uint32_t*>(p2 + 256 + 4 * i);
            const float d = h2f((uint16_t)(dd & 0xFFFFu)), dmin = h2f((uint16_t)(dd >> 16));
            const int j = c >> 5;
            const float sc = (float)p2[16 * i + j], mn = (float)p2[16 * i + 8 + j];
            w = __fsub_rn(__fmul_rn(__fmul_rn(d, sc), (float)q), __fmul_rn(dmin, mn));
        }
        out[(size_t)row * in + col] = w;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// the GEMV
// ------------------------------------------------------------------------------------------------------------------
constexpr int RP_MAXQ = 8;     // super-blocks of x one wave converts in the prologue (register quads)
#ifndef NTK_RP_LAZY_MIN
#define NTK_RP_LAZY_MIN 3   // quads of x per wave from which they are converted on the way (tuning builds: -DNTK_RP_LAZY_MIN=n)
#endif
#ifndef NTK_RP_DEPTH
#define NTK_RP_DEPTH 2
#endif
constexpr int RP_DEPTH = NTK_RP_DEPTH;    // items in flight per wave (tuning builds: -DNTK_RP_DEPTH=n)

struct RpSeg {
    const uint8_t* rp;   // repacked tensor (P1, then P2 at p2_off)
    float* y;
    size_t p2_off;
    int rows, tiles;
    int wg0, nwg;        // workgroups [wg0, wg0 + nwg) of the grid work on this segment
    int kb, krem;        // workgroup wl owns kb + (wl < krem) tiles (pairs of tiles in the SiLU form) from wl * kb + min(wl, krem)
};
// Timeline of a launch (trace builds only, make trace: -DNTK_GEMV_TRACE; tools/gemv_trace.py --rp): thread 0 of every workgroup stamps the
// constant 100 MHz clock at the phase boundaries of rp_body; read back with ntk_debug_rp_trace().
#ifdef NTK_GEMV_TRACE
constexpr int RT_SLOTS = 64, RT_WG = 512, RT_EV = 12;
__device__ unsigned long long g_rp_trace[RT_SLOTS][RT_WG][RT_EV];
#define RP_STAMP(ev) do { asm volatile("" ::: "memory"); rp_t[ev] = __builtin_amdgcn_s_memrealtime(); asm volatile("" ::: "memory"); } while (0)
#else
#define RP_STAMP(ev) do {} while (0)
#endif

struct RpParams {
    RpSeg seg[3];
    int nseg, nseg_a;    // segments [0, nseg_a) have the kernel's format A, the rest format B
    const float* x;
    int in, nsb;         // columns, super-blocks per row
    const float* norm_w;
    float eps;
    const float* resid;
    int silu_pair;       // seg[0] = gate, seg[1] = up (same shape, same format); their workgroups are seg[0]'s
#ifdef NTK_GEMV_TRACE
    int trace_slot;      // trace builds: which record of g_rp_trace this launch fills
#endif
};

// LDS: [0, 4 in) digit planes 0..2 + a plane of zeros | sub-block-sum digits, 64 B per super-block | 2^(e-22) per super-block |
//      32 floats scratch | row sums [tiles of the workgroup][waves][64 lanes]
__host__ __device__ inline size_t rp_lds_bytes(int in, int nsb, int nwaves, int ntl) {
    return (size_t)4 * in + (size_t)68 * nsb + 128 + (size_t)ntl * nwaves * 256 + 64;
}

__device__ __forceinline__ int dpp_add_i(int v, int src) { return v + src; }
template <int CTRL> __device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false); }

// one super-block of x (the wave's 256 columns, 4 per lane) -> digit planes, sub-block-sum digits, 2^(e-22)
template <int NSUB>
__device__ __forceinline__ void rp_convert_quad(uint8_t* smem, const int in, const int nsb, const int sb, const int lane, const float v0, const float v1,
                                                const float v2, const float v3) {
    float am = fmaxf(fmaxf(fabsf(v0), fabsf(v1)), fmaxf(fabsf(v2), fabsf(v3)));
    am = wave_max(am);
    int e = am > 0.0f ? __builtin_amdgcn_frexp_expf(am) : 0;   // am = m 2^e, 0.5 <= m < 1
    e = max(e, -100);                                            // (keeps 2^(22-e) finite for vanishing activations)
    const float up = __builtin_ldexpf(1.0f, 22 - e), inv = __builtin_ldexpf(1.0f, e - 22);
    // rint through the magic constant 1.5 * 2^23: the low mantissa bits ARE the two's-complement integer X, |X| <= 2^22.  Signed base-256
    // digits: X + 0x808080 has the digits d_p + 128 as its (unsigned) bytes -- one subtraction takes the magic constant off and puts the
    // bias on -- and an xor with 0x80 per byte (after the transpose, a dword at a time) makes them the int8 d_p
    const uint32_t y0 = __float_as_uint(fmaf(v0, up, 12582912.0f)) - (0x4B400000u - 0x808080u), y1 = __float_as_uint(fmaf(v1, up, 12582912.0f)) - (0x4B400000u - 0x808080u),
                   y2 = __float_as_uint(fmaf(v2, up, 12582912.0f)) - (0x4B400000u - 0x808080u), y3 = __float_as_uint(fmaf(v3, up, 12582912.0f)) - (0x4B400000u - 0x808080u);
    // 4 x 3 byte transpose: plane p of the four columns
    const uint32_t ta = __builtin_amdgcn_perm(y1, y0, 0x05010400u);    // y0.b0 y1.b0 y0.b1 y1.b1
    const uint32_t tb = __builtin_amdgcn_perm(y1, y0, 0x07030602u);    // y0.b2 y1.b2 y0.b3 y1.b3
    const uint32_t tc = __builtin_amdgcn_perm(y3, y2, 0x05010400u);
    const uint32_t td = __builtin_amdgcn_perm(y3, y2, 0x07030602u);
    const uint32_t p0 = __builtin_amdgcn_perm(tc, ta, 0x05040100u) ^ 0x80808080u;    // digit 0 of columns 0..3
    const uint32_t p1 = __builtin_amdgcn_perm(tc, ta, 0x07060302u) ^ 0x80808080u;    // digit 1
    const uint32_t p2 = __builtin_amdgcn_perm(td, tb, 0x05040100u) ^ 0x80808080u;    // digit 2
    const int col = 256 * sb + 4 * lane;
    *reinterpret_cast<uint32_t*>(smem + col) = p0;
    *reinterpret_cast<uint32_t*>(smem + in + col) = p1;
    *reinterpret_cast<uint32_t*>(smem + 2 * in + col) = p2;
    *reinterpret_cast<uint32_t*>(smem + 3 * in + col) = 0u;
    // sums of X over the 16-column (Q6_K) / 32-column (Q4_K, Q5_K) sub-blocks: 4 / 8 consecutive lanes
    int sm = (int)((y0 + y1) + (y2 + y3));   // (each term carries the bias 0x808080: 16 / 32 of them per sub-block, taken off below)
    sm += dpp_i<DPP_QUAD_1032>(sm);
    sm += dpp_i<DPP_QUAD_2301>(sm);
    if constexpr (NSUB == 8) sm += dpp_i<DPP_ROW_HALF_MIRROR>(sm);
    uint32_t ys = ((uint32_t)sm + (0x80808080u - (NSUB == 8 ? 32u : 16u) * 0x808080u)) ^ 0x80808080u;   // four signed digits (|sum| <= 2^27)
    int pos;
    if constexpr (NSUB == 8) { pos = (lane & 4) ? 8 + (lane >> 3) : (lane >> 3); if (lane & 4) ys = 0u; }   // bytes 8..15 of an entry stay zero
    else pos = lane >> 2;
    if ((lane & 3) == 0) {
        uint8_t* e0 = smem + 4 * (size_t)in + 64 * sb + pos;
        e0[0] = (uint8_t)ys; e0[16] = (uint8_t)(ys >> 8); e0[32] = (uint8_t)(ys >> 16); e0[48] = (uint8_t)(ys >> 24);
    }
    if (lane == 0) reinterpret_cast<float*>(smem + 4 * (size_t)in + 64 * (size_t)nsb)[sb] = inv;
}

template <int DT> struct RpItem {
    u4 n0, n1;      // the two step records' nibble chunks
    u4 rec;         // the row record
    uint32_t dd;    // d | dmin << 16  (Q6_K: d)
    uint32_t hb0, hb1;   // Q5_K
    u2 hh0, hh1;         // Q6_K
};

template <int DT, bool NORM>
__device__ __forceinline__ void rp_body(const RpParams& p, const int seg_lo, const int seg_hi, uint8_t* smem) {
    using F = Rp<DT>;
    constexpr int NSUB = F::NSUB;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int NW = (int)(blockDim.x >> 6);
    const int in = p.in, nsb = p.nsb;
    const int bid = (int)blockIdx.x;
#ifdef NTK_GEMV_TRACE
    unsigned long long rp_t[RT_EV] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    RP_STAMP(0);   // entry

    // ---- x (and the norm weights) first: everything below runs under their latency ----
    float4 xq[RP_MAXQ], wq[RP_MAXQ];
#pragma unroll
    for (int q = 0; q < RP_MAXQ; ++q) {
        xq[q] = float4{0.0f, 0.0f, 0.0f, 0.0f};
        wq[q] = float4{0.0f, 0.0f, 0.0f, 0.0f};
        const int sb = wave + q * NW;
        if (q * NW < nsb) {   // uniform
            const int col = min(sb, nsb - 1) * 256 + 4 * lane;
            xq[q] = *reinterpret_cast<const float4*>(p.x + col);
            if constexpr (NORM) wq[q] = *reinterpret_cast<const float4*>(p.norm_w + col);
        }
    }

    // ---- this workgroup's segment and tiles; the workgroup's items (tile x super-block, in memory order) go round the waves: at any
    //      moment the waves of a workgroup read ONE contiguous run of items (a wave that owned a contiguous range of its own would put
    //      every wave of the chip on the same offset of a power-of-two stride: measured, the 2 KiB-item Q4_K ran at 69 % of HBM where
    //      the 3 KiB-item Q6_K reached 81 %) ----
    RpSeg sg = p.seg[seg_lo];
    for (int k = seg_lo + 1; k < seg_hi; ++k)
        if (!p.silu_pair && bid >= p.seg[k].wg0) sg = p.seg[k];
    const bool silu = p.silu_pair != 0;
    const uint8_t* rp_alt = silu ? p.seg[1].rp : sg.rp;   // the up matrix (odd virtual tiles)
    const int mult = silu ? 2 : 1;
    const int wl = bid - sg.wg0;
    const int u0 = wl * sg.kb + min(wl, sg.krem), u1 = u0 + sg.kb + (wl < sg.krem ? 1 : 0);   // tiles (pairs) of this workgroup
    const int ntl = (u1 - u0) * mult;                 // virtual tiles (SiLU form: gate tile, up tile, gate tile ...)
    const int N = ntl * nsb;                          // items; wave w owns items w, w + NW, w + 2 NW ...
    const int i16 = lane & 15, kg = lane >> 4;

    // load cursor: item index and its virtual tile
    int l_idx = wave, l_v = 0;
    auto load_item = [&](RpItem<DT>& it) {   // the item under the load cursor (beyond the end: the workgroup's last item again -- an L2 hit)
        while (l_idx >= (l_v + 1) * nsb && l_v + 1 < ntl) ++l_v;   // uniform, at most a few steps
        const int li = min(l_idx, N - 1);
        const int tile = u0 + (silu ? (l_v >> 1) : l_v);
        const uint8_t* base = (silu && (l_v & 1)) ? rp_alt : sg.rp;
        const unsigned off = (unsigned)tile * (unsigned)nsb + (unsigned)(li - l_v * nsb);
        const uint8_t* p1 = base + (size_t)off * (2 * F::S1);
        const uint8_t* p2 = base + sg.p2_off + (size_t)off * F::S2;
        it.n0 = __builtin_nontemporal_load(reinterpret_cast<const u4*>(p1 + 16 * lane));
        it.n1 = __builtin_nontemporal_load(reinterpret_cast<const u4*>(p1 + F::S1 + 16 * lane));
        if constexpr (DT == NTK_DT_Q5_K) {
            it.hb0 = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p1 + 1024 + 4 * lane));
            it.hb1 = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p1 + F::S1 + 1024 + 4 * lane));
        }
        if constexpr (DT == NTK_DT_Q6_K) {
            it.hh0 = __builtin_nontemporal_load(reinterpret_cast<const u2*>(p1 + 1024 + 8 * lane));
            it.hh1 = __builtin_nontemporal_load(reinterpret_cast<const u2*>(p1 + F::S1 + 1024 + 8 * lane));
        }
        // (non-temporal like the rest of the weight stream: 12 % of the bytes must not push the KV cache and the activations out of L2)
        it.rec = __builtin_nontemporal_load(reinterpret_cast<const u4*>(p2 + 16 * i16));
        if constexpr (DT == NTK_DT_Q6_K) it.dd = __builtin_nontemporal_load(reinterpret_cast<const uint16_t*>(p2 + 256 + 2 * i16));
        else it.dd = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(p2 + 256 + 4 * i16));
        l_idx += NW;
    };

    // The weights are requested right BEHIND x, without waiting for it to land (a CU returns its loads in request order: x, requested
    // first, still arrives first).  gemv.hip waits for x before its first weight row and gains from it (there a wave's x request is one of
    // 8 / 16 that the whole workgroup's image needs, and a late wave's request queues behind the early waves' rows); here a wave needs only
    // its OWN two to seven quads, and the wait was a round trip added to every launch: without it 8B Q4_K_M decodes 675 -> 709-714 tok/s,
    // Wo 5.02 -> 4.77 us, 70B down 24.5 -> 24.0 (same-box A/B, twice alternated: profiles/r04_gemv_rp_epilogue_experiment.txt).
    // -DNTK_RP_XWAIT (tuning experiments): the former order.
#ifdef NTK_RP_XWAIT
#pragma unroll
    for (int q = 0; q < RP_MAXQ; ++q) asm volatile("" : "+v"(xq[q].x), "+v"(xq[q].y), "+v"(xq[q].z), "+v"(xq[q].w));
#endif
    // RP_DEPTH items on their way, UNCONDITIONALLY (the s_waitcnt of the steady-state loop is exact only if its entry state is)
    RpItem<DT> ring[RP_DEPTH];
    RP_STAMP(1);   // x requested, row bookkeeping done
#pragma unroll
    for (int u = 0; u < RP_DEPTH; ++u) load_item(ring[u]);
    RP_STAMP(2);   // first items requested

    // ---- prologue: RMSNorm (reference rmsnorm.cu:16-70), digit planes ----
    float* red = reinterpret_cast<float*>(smem + 4 * (size_t)in + 68 * (size_t)nsb);
    float* part = red + 32;
    if constexpr (NORM) {
        float ssq = 0.0f;
#pragma unroll
        for (int q = 0; q < RP_MAXQ; ++q) {
            const float m = (wave + q * NW < nsb) ? 1.0f : 0.0f;
            ssq = fmaf(xq[q].x * m, xq[q].x, ssq); ssq = fmaf(xq[q].y * m, xq[q].y, ssq);
            ssq = fmaf(xq[q].z * m, xq[q].z, ssq); ssq = fmaf(xq[q].w * m, xq[q].w, ssq);
        }
        ssq = wave_sum(ssq);
        if (lane == 0) red[wave] = ssq;
        __syncthreads();
        float tot = 0.0f;
        for (int w = 0; w < NW; ++w) tot += red[w];
        const float rms_inv = 1.0f / sqrtf(tot / (float)in + p.eps);   // rsqrtf(mean + eps), rmsnorm.cu:60-61
#pragma unroll
        for (int q = 0; q < RP_MAXQ; ++q) {   // x * rms_inv * w, the reference's association (rmsnorm.cu:68)
            xq[q].x = xq[q].x * rms_inv * wq[q].x; xq[q].y = xq[q].y * rms_inv * wq[q].y;
            xq[q].z = xq[q].z * rms_inv * wq[q].z; xq[q].w = xq[q].w * rms_inv * wq[q].w;
        }
    }
    // The digit image.  When the waves divide the super-blocks evenly (or the workgroup has one tile), wave w only ever decodes super-blocks w,
    // w + NW ...: exactly the ones whose x it holds -- its part of the image is private: no barrier, and each quad is converted right
    // before the first item that needs it (process(), first tile), so the weight stream keeps flowing under the conversion (~70 VALU
    // instructions per quad: 4 us of a CU's time for the 28672 columns of the 70B down projection when done up front).  Until then the
    // quad waits IN PLACE: component c of lane l in the bytes of plane c it will overwrite.  Otherwise: all of it now, barrier.
    // (measured, tools/gemv_bench.py: with 4 / 7 quads per wave -- the 8192- and 28672-column launches -- on-the-way conversion gains
    // 0.5 ... 2.3 us per launch; with 2 -- 4096 columns -- the trip through LDS costs 0.25 us more than it hides: those convert at once)
    const bool priv = nsb % NW == 0 || ntl == 1;     // uniform (one tile: item index = super-block index, whatever the remainder)
    const int nq = (priv && (nsb + NW - 1) / NW >= NTK_RP_LAZY_MIN) ? (nsb + NW - 1) / NW : 0;   // quads converted on the way
#pragma unroll
    for (int q = 0; q < RP_MAXQ; ++q) {
        const int sb = wave + q * NW;
        if (sb < nsb) {   // uniform
            if (nq > 0 && q > 0) {
                uint8_t* at = smem + 256 * sb + 4 * lane;
                *reinterpret_cast<float*>(at) = xq[q].x; *reinterpret_cast<float*>(at + in) = xq[q].y;
                *reinterpret_cast<float*>(at + 2 * in) = xq[q].z; *reinterpret_cast<float*>(at + 3 * in) = xq[q].w;
            } else {
                rp_convert_quad<NSUB>(smem, in, nsb, sb, lane, xq[q].x, xq[q].y, xq[q].z, xq[q].w);
            }
        }
    }
    if (!priv) __syncthreads();
    RP_STAMP(3);   // x landed, (RMSNorm,) digit image of the first quad(s) written

    // ---- lane constants of the A operands (digit planes) ----
    const int m16 = lane & 15;            // entry m = 4 jj + p of the first MFMA operand
    const int jjm = m16 >> 2, pp = m16 & 3;
    const bool a_ok = pp < 3 && (NSUB == 8 ? (jjm == (kg >> 1)) : (jjm == kg));
    const uint32_t xbase = (uint32_t)(a_ok ? pp * in : 3 * in) + 16u * (uint32_t)kg;
    const bool c_ok = m16 < 4 && kg == 0;   // correction: entry m = digit m of the sub-block sums, k-slots of kg 0 only
    const uint32_t cbase = c_ok ? (uint32_t)(4 * in + 16 * m16) : (uint32_t)(3 * in);
    const uint32_t cstride = c_ok ? 64u : 256u;   // (the other lanes read zeros of THEIR item's super-block: written by this wave)
    const float* invt = reinterpret_cast<const float*>(smem + 4 * (size_t)in + 64 * (size_t)nsb);
    const uint32_t o0 = 8u * (uint32_t)kg, o1 = o0 + 16u;   // bit offsets of this lane's scale byte in a dword of the row record

    float racc = 0.0f;
    int p_idx = wave, p_tl = 0;            // process cursor: item index, virtual tile being accumulated
    auto flush = [&]() {                   // this wave's share of tile p_tl (zero if it had no item there): 64 lane sums, added up in the epilogue
        part[(p_tl * NW + wave) * 64 + lane] = racc;
        racc = 0.0f;
        ++p_tl;
    };

    const v4i z4 = {0, 0, 0, 0};
    auto process = [&](const RpItem<DT>& it) {
        while (p_idx >= (p_tl + 1) * nsb) flush();   // uniform
        const int sbk = p_idx - p_tl * nsb;
        p_idx += NW;
        if (nq > 0 && p_tl == 0 && sbk >= NW) {   // first use of this super-block's x (uniform): floats in place -> digit planes (LDS and VALU only)
            const uint8_t* at = smem + 256 * sbk + 4 * lane;
            const float v0 = *reinterpret_cast<const float*>(at), v1 = *reinterpret_cast<const float*>(at + in);
            const float v2 = *reinterpret_cast<const float*>(at + 2 * in), v3 = *reinterpret_cast<const float*>(at + 3 * in);
            rp_convert_quad<NSUB>(smem, in, nsb, sbk, lane, v0, v1, v2, v3);
        }
        const uint8_t* xa = smem + xbase + 256u * (uint32_t)sbk;
        v4i b[4];
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const u4 raw = s ? it.n1 : it.n0;
            v4i& b0 = b[2 * s];
            v4i& b1 = b[2 * s + 1];
            if constexpr (DT == NTK_DT_Q4_K) {
#pragma unroll
                for (int k = 0; k < 4; ++k) { b0[k] = (int)(raw[k] & 0x0F0F0F0Fu); b1[k] = (int)((raw[k] >> 4) & 0x0F0F0F0Fu); }
            } else if constexpr (DT == NTK_DT_Q5_K) {
                const uint32_t hb = s ? it.hb1 : it.hb0;   // byte y, bit 4 h + v
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    b0[k] = (int)(((hb << (4 - k)) & 0x10101010u) | (raw[k] & 0x0F0F0F0Fu));
                    b1[k] = (int)(((hb >> k) & 0x10101010u) | ((raw[k] >> 4) & 0x0F0F0F0Fu));
                }
            } else {
                const u2 hh = s ? it.hh1 : it.hh0;         // byte y, bits 2 v .. 2 v + 1
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t h0 = k < 2 ? (hh[0] << (4 - 2 * k)) : (hh[0] >> (2 * k - 4));
                    const uint32_t h1 = k < 2 ? (hh[1] << (4 - 2 * k)) : (hh[1] >> (2 * k - 4));
                    b0[k] = (int)((h0 & 0x30303030u) | (raw[k] & 0x0F0F0F0Fu));
                    b1[k] = (int)((h1 & 0x30303030u) | ((raw[k] >> 4) & 0x0F0F0F0Fu));
                }
            }
        }
        // minimum (Q4_K / Q5_K: dmin sum_j m_j sum x) / offset (Q6_K: 32 d sum_j sc_j sum x) term: the row's bytes x the digits of the sums
        v4i bc;
        if constexpr (NSUB == 8) bc = v4i{kg == 0 ? (int)it.rec[2] : 0, kg == 0 ? (int)it.rec[3] : 0, 0, 0};
        else bc = v4i{kg == 0 ? (int)it.rec[0] : 0, kg == 0 ? (int)it.rec[1] : 0, kg == 0 ? (int)it.rec[2] : 0, kg == 0 ? (int)it.rec[3] : 0};
        const v4i a0 = *reinterpret_cast<const v4i*>(xa), a1 = *reinterpret_cast<const v4i*>(xa + 64);
        const v4i a2 = *reinterpret_cast<const v4i*>(xa + 128), a3 = *reinterpret_cast<const v4i*>(xa + 192);
        const v4i ac = *reinterpret_cast<const v4i*>(smem + cbase + cstride * (uint32_t)sbk);
        const float inv = invt[sbk];
        // the five matrix instructions back to back; their results are consumed below, after the last has been issued
        const v4i c0 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a0, b[0], z4, 0, 0, 0);
        const v4i c1 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a1, b[1], z4, 0, 0, 0);
        const v4i c2 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a2, b[2], z4, 0, 0, 0);
        const v4i c3 = __builtin_amdgcn_mfma_i32_16x16x64_i8(a3, b[3], z4, 0, 0, 0);
        const v4i cc = __builtin_amdgcn_mfma_i32_16x16x64_i8(ac, bc, z4, 0, 0, 0);
        int s0, s1, s2, s3;   // the scale of (row, sub-block of this lane) in each of the four MFMAs
        if constexpr (NSUB == 8) {   // sub-block 4 s + 2 h + mg: byte 2 h + mg of dword s of the record
            s0 = (int)__builtin_amdgcn_ubfe(it.rec[0], o0, 8u); s1 = (int)__builtin_amdgcn_ubfe(it.rec[0], o1, 8u);
            s2 = (int)__builtin_amdgcn_ubfe(it.rec[1], o0, 8u); s3 = (int)__builtin_amdgcn_ubfe(it.rec[1], o1, 8u);
        } else {                     // sub-block 8 s + 4 h + mg: byte mg of dword 2 s + h
            s0 = __builtin_amdgcn_sbfe((int)it.rec[0], o0, 8u); s1 = __builtin_amdgcn_sbfe((int)it.rec[1], o0, 8u);
            s2 = __builtin_amdgcn_sbfe((int)it.rec[2], o0, 8u); s3 = __builtin_amdgcn_sbfe((int)it.rec[3], o0, 8u);
        }
        const int i0 = __mul24(c0[0], s0) + __mul24(c1[0], s1) + __mul24(c2[0], s2) + __mul24(c3[0], s3);
        const int i1 = __mul24(c0[1], s0) + __mul24(c1[1], s1) + __mul24(c2[1], s2) + __mul24(c3[1], s3);
        const int i2 = __mul24(c0[2], s0) + __mul24(c1[2], s1) + __mul24(c2[2], s2) + __mul24(c3[2], s3);
        const float d = h2f((uint16_t)(it.dd & 0xFFFFu));
        const float S = fmaf(fmaf((float)i2, 256.0f, (float)i1), 256.0f, (float)i0);
        racc = fmaf(S, d * inv, racc);
        const float corr = fmaf(fmaf(fmaf((float)cc[3], 256.0f, (float)cc[2]), 256.0f, (float)cc[1]), 256.0f, (float)cc[0]);
        float fneg;
        if constexpr (NSUB == 8) fneg = -h2f((uint16_t)(it.dd >> 16)) * inv; else fneg = -32.0f * d * inv;
        racc = fmaf(corr, fneg, racc);
    };

    // ---- the wave's items: RP_DEPTH in flight; the steady-state loop issues unconditionally (exact s_waitcnt), the tail does not ----
    // (p_idx: next item to process; items p_idx, p_idx + NW ... p_idx + (RP_DEPTH - 1) NW are in the ring)
    while (p_idx + (2 * RP_DEPTH - 1) * NW < N) {   // the prefetches of this trip (items + RP_DEPTH ... + 2 RP_DEPTH - 1) all exist
#pragma unroll
        for (int u = 0; u < RP_DEPTH; ++u) { process(ring[u]); load_item(ring[u]); }
    }
    RP_STAMP(4);   // steady-state loop done (all items but the last 2 RP_DEPTH of wave 0)
#pragma unroll
    for (int u = 0; u < RP_DEPTH; ++u)
        if (p_idx < N) { process(ring[u]); if (p_idx + (RP_DEPTH - 1) * NW < N) load_item(ring[u]); }
#pragma unroll
    for (int u = 0; u < RP_DEPTH; ++u)
        if (p_idx < N) process(ring[u]);
#ifdef NTK_GEMV_TRACE
    asm volatile("" :: "v"(racc));
#endif
    RP_STAMP(5);   // wave 0's last item accumulated
#ifndef NTK_RP_RESID_EPILOGUE
    // The residual of the row this thread stores, requested HERE: behind the item loop (requested in the prologue it made hipcc's counted
    // waits of the loop conservative and lost 3 %, profiles/NEGATIVE_RESULTS.md section 6), in front of the flush and the barrier, whose
    // time the L2 round trip then overlaps.  Round 5, same-box A/B alternated three times (profiles/r05_ab_variants.txt): +0.4 % alone,
    // +2.3 % together with the kernel-argument touch below (8B Q4_K_M 711 -> 728 tok/s).  -DNTK_RP_RESID_EPILOGUE: the former order.
    float res_late = 0.0f;
    {
        const bool res_l = !silu && p.resid != nullptr && sg.wg0 == p.seg[0].wg0;
        const int row_l = (u0 + (tid >> 4)) * 16 + (tid & 15);
        if (res_l && tid < ntl * 16 && row_l < sg.rows) res_late = p.resid[row_l];
    }
#endif
    while (p_tl < ntl) flush();
    __syncthreads();
    RP_STAMP(6);   // every wave's share is in LDS

    // ---- row sums of the workgroup's tiles: the waves' shares in wave order (and the four sub-block lanes of a row), epilogue, store ----
    // (round 6: the shares of EIGHT waves are requested before the first is added -- the rolled loop over a run-time wave count was one LDS round trip per wave,
    // ~0.45 us between the barrier and the store in the launch timeline, profiles/r06_gemv_rp_timeline.txt; the additions keep their order: identical bits.
    // -DNTK_RP_EPILOGUE_ROLLED: the former loop)
    auto tile_sum = [&](const int tl, const int r) {
        const float* q = part + (size_t)tl * NW * 64 + r;
        float t = 0.0f;
        int w = 0;
#ifndef NTK_RP_EPILOGUE_ROLLED
        for (; w + 8 <= NW; w += 8) {
            float a[8][4];
#pragma unroll
            for (int k = 0; k < 8; ++k) { a[k][0] = q[(w + k) * 64]; a[k][1] = q[(w + k) * 64 + 16]; a[k][2] = q[(w + k) * 64 + 32]; a[k][3] = q[(w + k) * 64 + 48]; }
#pragma unroll
            for (int k = 0; k < 8; ++k) t += (a[k][0] + a[k][1]) + (a[k][2] + a[k][3]);
        }
#endif
        for (; w < NW; ++w) t += (q[w * 64] + q[w * 64 + 16]) + (q[w * 64 + 32] + q[w * 64 + 48]);
        return t;
    };
    if (silu) {
        for (int e = tid; e < (u1 - u0) * 16; e += (int)blockDim.x) {
            const int pl = e >> 4, r = e & 15, row = (u0 + pl) * 16 + r;
            if (row < sg.rows) {
                const float gv = tile_sum(2 * pl, r), uv = tile_sum(2 * pl + 1, r);
                sg.y[row] = gv / (1.0f + expf(-gv)) * uv;   // reference gemm.cu:719-724
            }
        }
    } else {
        const bool res = p.resid != nullptr && sg.wg0 == p.seg[0].wg0;   // the residual belongs to segment 0
        for (int e = tid; e < ntl * 16; e += (int)blockDim.x) {
            const int tl = e >> 4, r = e & 15, row = (u0 + tl) * 16 + r;
            if (row < sg.rows) {
                float v = tile_sum(tl, r);
#ifndef NTK_RP_RESID_EPILOGUE
                if (res) v = (e == tid ? res_late : p.resid[row]) + v;   // reference elementwise.cu:23-32
#else
                if (res) v = p.resid[row] + v;   // reference elementwise.cu:23-32
#endif
                sg.y[row] = v;
            }
        }
    }
    RP_STAMP(7);   // results stored (requests issued)
#ifdef NTK_GEMV_TRACE
    if (tid == 0 && bid < RT_WG) {
        rp_t[8] = (unsigned long long)N; rp_t[9] = (unsigned long long)NW;
        for (int e = 0; e < RT_EV; ++e) g_rp_trace[p.trace_slot & (RT_SLOTS - 1)][bid][e] = rp_t[e];
    }
#endif
}

template <int DTA, int DTB, bool NORM>
__global__ __launch_bounds__(1024) void rp_gemv_kernel(const RpParams p) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rp_smem[];
#ifndef NTK_RP_NO_KERNARG_TOUCH
    {
        // RpParams is four kernel-argument cache lines; hipcc fetches x / in (line 2-3) first and the segment table (line 0) only in front
        // of the first weight request: a second scalar-cache miss between the x requests and the weight requests (ISA of
        // rp_gemv_kernel<Q4_K, Q4_K, false>: s_waitcnt lgkmcnt(0) at instruction 120, first weight load at 362).  Touching all four lines
        // at once: 8B Q4_K_M 711 -> 726 tok/s (+2.0 %, round 5 same-box A/B alternated three times, profiles/r05_ab_variants.txt);
        // gemv.hip does the same and gains 0.7 % from it.
        const auto* ka = __builtin_amdgcn_kernarg_segment_ptr();
        unsigned d0, d1, d2, d3;
        asm volatile("s_load_dword %0, %4, 0x0\n\ts_load_dword %1, %4, 0x40\n\ts_load_dword %2, %4, 0x80\n\ts_load_dword %3, %4, 0xc0\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&s"(d0), "=&s"(d1), "=&s"(d2), "=&s"(d3) : "s"(ka) : "memory");
        __builtin_amdgcn_sched_barrier(0);
    }
#endif
    if constexpr (DTA == DTB) {
        rp_body<DTA, NORM>(p, 0, p.nseg, rp_smem);
    } else {
        if ((int)blockIdx.x < p.seg[p.nseg_a].wg0) rp_body<DTA, NORM>(p, 0, p.nseg_a, rp_smem);
        else rp_body<DTB, NORM>(p, p.nseg_a, p.nseg, rp_smem);
    }
}

// prologue only: the LDS image of x (4 in + 68 nsb bytes) to global memory.  Parity instrumentation.
template <int NSUB, bool NORM>
__global__ __launch_bounds__(1024) void rp_prologue_dump_kernel(uint8_t* out, const float* x, const float* norm_w, float eps, int in, int nsb) {
    extern __shared__ __attribute__((aligned(16))) uint8_t rp_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NW = blockDim.x >> 6;
    float* red = reinterpret_cast<float*>(rp_smem + 4 * (size_t)in + 68 * (size_t)nsb);
    float rms_inv = 1.0f;
    if (NORM) {
        float ssq = 0.0f;
        for (int c = tid; c < in; c += blockDim.x) ssq = fmaf(x[c], x[c], ssq);
        ssq = wave_sum(ssq);
        if (lane == 0) red[wave] = ssq;
        __syncthreads();
        float tot = 0.0f;
        for (int w = 0; w < NW; ++w) tot += red[w];
        rms_inv = 1.0f / sqrtf(tot / (float)in + eps);
    }
    for (int sb = wave; sb < nsb; sb += NW) {
        float4 v = *reinterpret_cast<const float4*>(x + 256 * sb + 4 * lane);
        if (NORM) {
            const float4 w = *reinterpret_cast<const float4*>(norm_w + 256 * sb + 4 * lane);
            v.x = v.x * rms_inv * w.x; v.y = v.y * rms_inv * w.y; v.z = v.z * rms_inv * w.z; v.w = v.w * rms_inv * w.w;
        }
        rp_convert_quad<NSUB>(rp_smem, in, nsb, sb, lane, v.x, v.y, v.z, v.w);
    }
    __syncthreads();
    const size_t n = 4 * (size_t)in + 68 * (size_t)nsb;
    for (size_t k = tid; k < n; k += blockDim.x) out[k] = rp_smem[k];
}

// D = A . B on v_mfma_i32_16x16x64_i8 with the operand / accumulator lane maps the GEMV assumes (A [16][64], B [64][16] -> D [16][16]):
// first operand lane (i = lane & 15, kg = lane >> 4) = A[i][16 kg .. 16 kg + 15], second = B[16 kg ..][j = lane & 15], result lane
// (j = lane & 15, mg = lane >> 4) register r = D[4 mg + r][j].  Parity instrumentation (a wrong map fails this before anything else).
__global__ __launch_bounds__(64) void rp_mfma_probe_kernel(int* D, const int8_t* A, const int8_t* B) {
    const int lane = threadIdx.x, i = lane & 15, kg = lane >> 4;
    v4i a, b;
    int8_t ta[16], tb[16];
    for (int k = 0; k < 16; ++k) { ta[k] = A[i * 64 + 16 * kg + k]; tb[k] = B[(16 * kg + k) * 16 + i]; }
    __builtin_memcpy(&a, ta, 16);
    __builtin_memcpy(&b, tb, 16);
    const v4i z = {0, 0, 0, 0};
    const v4i c = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, z, 0, 0, 0);
    for (int r = 0; r < 4; ++r) D[(4 * kg + r) * 16 + i] = c[r];
}

// ------------------------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------------------------
struct RpPlan { int nw, grid; size_t lds; int nwg[3]; };

// Geometry of one launch.  A workgroup owns whole tiles (pairs of tiles for the SiLU form) of ONE segment; its items (tile x super-block)
// go round its waves, which meet in LDS.  Workgroups land on CUs round-robin, so what a launch costs is (the most loaded CU's bytes) +
// (a prologue per workgroup).  Rules, from sweeps of every (waves per workgroup, workgroups per CU) at the 8B / 70B shapes
// (tools/gemv_bench.py --rp --sweep, profiles/r04_gemv_rp_plan_sweep.txt):
//   * 8 waves per workgroup; 16 when x has more than 32 super-blocks (the down projections).  (14 waves for the 56 super-blocks of the
//     8B down projection, which would keep every wave's part of the digit image private, measured slower than 16 with a barrier.)
//   * one workgroup per CU, k = ceil(units / 256) units each -- unless two workgroups of ceil(units / 512) units load the fullest CU no
//     more AND that grid would leave a sixth of the CUs of a long launch (>= 48 MB) idle (the 8B gate|up: 224 workgroups of 4 pairs).
static bool rp_plan_try(const int* tiles, const int* dts, int nsegw, int mult, int nsb, int in, int nw, int per_cu, RpPlan& out, int* max_cu_units) {
    if ((nsb + nw - 1) / nw > RP_MAXQ || per_cu < 1 || per_cu * nw > 16) return false;
    const int gmax = 256 * per_cu;
    double wsum = 0.0;
    for (int i = 0; i < nsegw; ++i) wsum += (double)tiles[i] * (double)(2 * rp_s1(dts[i]) + rp_s2(dts[i]));
    int grid = 0, max_ntl = 0, kmax = 0;
    for (int i = 0; i < nsegw; ++i) {
        const double wi = (double)tiles[i] * (double)(2 * rp_s1(dts[i]) + rp_s2(dts[i]));
        int gi = std::max(1, (int)(gmax * wi / wsum));
        gi = std::min(gi, tiles[i]);
        const int k = (tiles[i] + gi - 1) / gi;           // tiles (pairs) per workgroup, at most
        gi = (tiles[i] + k - 1) / k;
        out.nwg[i] = gi;
        grid += gi;
        kmax = std::max(kmax, k);
        max_ntl = std::max(max_ntl, k * mult);
    }
    if (grid > gmax) return false;
    const size_t lds = rp_lds_bytes(in, nsb, nw, max_ntl);
    if (lds > 160 * 1024 || (size_t)per_cu * lds > 160 * 1024) return false;
    out.nw = nw; out.grid = grid; out.lds = lds;
    *max_cu_units = kmax * ((grid + 255) / 256);   // CU 0 hosts ceil(grid / 256) workgroups
    return true;
}

static bool rp_plan(const int* tiles, const int* dts, int nseg, int nsb, int in, int silu_pair, int force_nw, int force_per_cu, RpPlan& best) {
    const int mult = silu_pair ? 2 : 1;
    const int nsegw = silu_pair ? 1 : nseg;   // segments that own workgroups
    double bytes = 0.0;
    for (int i = 0; i < nsegw; ++i) bytes += (double)tiles[i] * mult * nsb * (double)(2 * rp_s1(dts[i]) + rp_s2(dts[i]));
    int m = 0;
    if (force_nw > 0 || force_per_cu > 0) {   // tuning builds
        for (int nw : {16, 14, 12, 10, 8, 7, 6, 5, 4}) for (int pc = 4; pc >= 1; --pc) {
            if ((force_nw > 0 && nw != force_nw) || (force_per_cu > 0 && pc != force_per_cu)) continue;
            if (rp_plan_try(tiles, dts, nsegw, mult, nsb, in, nw, pc, best, &m)) return true;
        }
        return false;
    }
    const int nw = nsb > 32 ? 16 : 8;
    RpPlan one, two;
    int m1 = 0, m2 = 0;
    const bool ok1 = rp_plan_try(tiles, dts, nsegw, mult, nsb, in, nw, 1, one, &m1);
    const bool ok2 = nw == 8 && rp_plan_try(tiles, dts, nsegw, mult, nsb, in, nw, 2, two, &m2);
    if (ok1 && ok2) { best = (m2 <= m1 && one.grid < 240 && bytes >= 48e6) ? two : one; return true; }
    if (ok1) { best = one; return true; }
    if (ok2) { best = two; return true; }
    for (int w : {16, 14, 12, 10, 8, 7, 6, 5, 4}) for (int pc = 1; pc <= 4; ++pc)   // whatever fits (shapes outside the target models)
        if (rp_plan_try(tiles, dts, nsegw, mult, nsb, in, w, pc, best, &m)) return true;
    return false;
}

static int g_rp_force_nw = 0, g_rp_force_per_cu = 0;   // tuning builds: ntk_tune_rp_plan()
static int g_rp_last_nw = 0, g_rp_last_grid = 0, g_rp_last_lds = 0;

using RpFn = void (*)(const RpParams);
template <int DTA, int DTB> static RpFn rp_fn(bool norm) {
    static const RpFn t[2] = {rp_gemv_kernel<DTA, DTB, false>, rp_gemv_kernel<DTA, DTB, true>};
    static const bool ok = hipFuncSetAttribute((const void*)t[0], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
                           hipFuncSetAttribute((const void*)t[1], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
    return ok ? t[norm ? 1 : 0] : nullptr;
}

}  // namespace ntk

extern "C" {

size_t ntk_rp_bytes(int dtype, int rows, int in_features) {
    if (!ntk::rp_supported(dtype) || rows <= 0 || in_features <= 0 || in_features % 256 != 0) return 0;
    const size_t tiles = ((size_t)rows + 15) / 16, nsb = (size_t)in_features / 256;
    return tiles * nsb * (2 * ntk::rp_s1(dtype) + ntk::rp_s2(dtype));
}

int ntk_rp_pack(void* dst, const void* raw, int rows, int in_features, int dtype, void* stream) {
    if (!dst || !raw) return NTK_E_NULL;
    if (!ntk::rp_supported(dtype)) return NTK_E_DTYPE;
    if (rows <= 0 || in_features <= 0 || in_features % 256 != 0) return NTK_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(dst) & 15) return NTK_E_ALIGN;
    const int tiles = (rows + 15) / 16, nsb = in_features / 256;
    if ((long)tiles * nsb > 0x7FFFFFFFl) return NTK_E_SHAPE;
    const size_t p2 = (size_t)tiles * nsb * 2 * ntk::rp_s1(dtype);
    hipStream_t st = ntk::resolve_stream(stream);
    const dim3 g((unsigned)(tiles * nsb)), b(128);
    uint8_t* d = static_cast<uint8_t*>(dst);
    const uint8_t* r = static_cast<const uint8_t*>(raw);
    if (dtype == NTK_DT_Q4_K) hipLaunchKernelGGL(ntk::rp_pack_kernel<NTK_DT_Q4_K>, g, b, 0, st, d, r, rows, nsb, p2);
    else if (dtype == NTK_DT_Q5_K) hipLaunchKernelGGL(ntk::rp_pack_kernel<NTK_DT_Q5_K>, g, b, 0, st, d, r, rows, nsb, p2);
    else hipLaunchKernelGGL(ntk::rp_pack_kernel<NTK_DT_Q6_K>, g, b, 0, st, d, r, rows, nsb, p2);
    return ntk::last_launch_status();
}

int ntk_rp_unpack(void* raw, const void* rp, int rows, int in_features, int dtype, void* stream) {
    if (!raw || !rp) return NTK_E_NULL;
    if (!ntk::rp_supported(dtype)) return NTK_E_DTYPE;
    if (rows <= 0 || in_features <= 0 || in_features % 256 != 0) return NTK_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(rp) & 15) || (reinterpret_cast<uintptr_t>(raw) & (dtype == NTK_DT_Q6_K ? 1 : 3))) return NTK_E_ALIGN;
    const int tiles = (rows + 15) / 16, nsb = in_features / 256;
    if ((long)tiles * nsb > 0x7FFFFFFFl) return NTK_E_SHAPE;
    const size_t p2 = (size_t)tiles * nsb * 2 * ntk::rp_s1(dtype);
    hipStream_t st = ntk::resolve_stream(stream);
    const dim3 g((unsigned)(tiles * nsb)), b(256);
    uint8_t* d = static_cast<uint8_t*>(raw);
    const uint8_t* r = static_cast<const uint8_t*>(rp);
    if (dtype == NTK_DT_Q4_K) hipLaunchKernelGGL(ntk::rp_unpack_kernel<NTK_DT_Q4_K>, g, b, 0, st, d, r, rows, nsb, p2);
    else if (dtype == NTK_DT_Q5_K) hipLaunchKernelGGL(ntk::rp_unpack_kernel<NTK_DT_Q5_K>, g, b, 0, st, d, r, rows, nsb, p2);
    else hipLaunchKernelGGL(ntk::rp_unpack_kernel<NTK_DT_Q6_K>, g, b, 0, st, d, r, rows, nsb, p2);
    return ntk::last_launch_status();
}

int ntk_rp_dequant(float* out, const void* rp, int rows, int in_features, int dtype, void* stream) {
    if (!out || !rp) return NTK_E_NULL;
    if (!ntk::rp_supported(dtype)) return NTK_E_DTYPE;
    if (rows <= 0 || in_features <= 0 || in_features % 256 != 0) return NTK_E_SHAPE;
    const int tiles = (rows + 15) / 16, nsb = in_features / 256;
    const size_t p2 = (size_t)tiles * nsb * 2 * ntk::rp_s1(dtype);
    hipStream_t st = ntk::resolve_stream(stream);
    const dim3 g((unsigned)rows), b(256);
    const uint8_t* r = static_cast<const uint8_t*>(rp);
    if (dtype == NTK_DT_Q4_K) hipLaunchKernelGGL(ntk::rp_dequant_kernel<NTK_DT_Q4_K>, g, b, 0, st, out, r, rows, in_features, nsb, p2);
    else if (dtype == NTK_DT_Q5_K) hipLaunchKernelGGL(ntk::rp_dequant_kernel<NTK_DT_Q5_K>, g, b, 0, st, out, r, rows, in_features, nsb, p2);
    else hipLaunchKernelGGL(ntk::rp_dequant_kernel<NTK_DT_Q6_K>, g, b, 0, st, out, r, rows, in_features, nsb, p2);
    return ntk::last_launch_status();
}

int ntk_gemv_rp_fused(const ntk_gemv_seg* segs, int nseg, const float* x, int in_features, const float* norm_w, float eps,
                      const float* resid, int silu_pair, void* stream) {
    using namespace ntk;
    if (!segs || !x) return NTK_E_NULL;
    if (nseg < 1 || nseg > 3) return NTK_E_SHAPE;
    if (in_features <= 0 || in_features % 256 != 0 || in_features > 32768) return NTK_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(x) & 15) || (norm_w && (reinterpret_cast<uintptr_t>(norm_w) & 15))) return NTK_E_ALIGN;
    if (silu_pair && (nseg != 2 || segs[0].rows != segs[1].rows || segs[0].dtype != segs[1].dtype || resid)) return NTK_E_SHAPE;
    {   // all-Q8_0 segment lists: W = the lane-major rows of ntk_q8l_pack, csrc/gemv.hip (Q8_0 beside a K-quant: not taken, NTK_E_DTYPE below)
        bool q8 = true;
        for (int i = 0; i < nseg; ++i) q8 = q8 && segs[i].dtype == NTK_DT_Q8_0;
        if (q8) {
            for (int i = 0; i < nseg; ++i) {
                if (segs[i].rows <= 0) return NTK_E_SHAPE;
                if (!segs[i].W || !segs[i].y) return NTK_E_NULL;
            }
            return q8l_gemv_fused(segs, nseg, x, in_features, norm_w, eps, resid, silu_pair, resolve_stream(stream));
        }
    }
    // order: format A first (the first segment's), then the rest (one other format at most)
    ntk_gemv_seg ord[3];
    int na = 0, nb = 0, dtb = -1;
    for (int i = 0; i < nseg; ++i) {
        if (!rp_supported(segs[i].dtype)) return NTK_E_DTYPE;
        if (segs[i].rows <= 0) return NTK_E_SHAPE;
        if (!segs[i].W || !segs[i].y) return NTK_E_NULL;
        if (reinterpret_cast<uintptr_t>(segs[i].W) & 15) return NTK_E_ALIGN;
    }
    for (int i = 0; i < nseg; ++i) if (segs[i].dtype == segs[0].dtype) ord[na++] = segs[i];
    for (int i = 0; i < nseg; ++i) if (segs[i].dtype != segs[0].dtype) {
        if (dtb < 0) dtb = segs[i].dtype; else if (segs[i].dtype != dtb) return NTK_E_DTYPE;
        ord[na + nb++] = segs[i];
    }
    if (resid && ord[0].W != segs[0].W) return NTK_E_SHAPE;   // (the residual belongs to segment 0, which is of format A by construction)
    const int dta = segs[0].dtype;
    if (dtb < 0) dtb = dta;
    RpParams p;
    memset(&p, 0, sizeof p);
    const int nsb = in_features / 256;
    int tiles[3] = {0, 0, 0}, dts[3] = {0, 0, 0};
    for (int i = 0; i < nseg; ++i) { tiles[i] = (ord[i].rows + 15) / 16; dts[i] = ord[i].dtype; }
    RpPlan plan;
    if (!rp_plan(tiles, dts, nseg, nsb, in_features, silu_pair, g_rp_force_nw, g_rp_force_per_cu, plan)) return NTK_E_SHAPE;
    int wg = 0;
    for (int i = 0; i < nseg; ++i) {
        RpSeg& s = p.seg[i];
        s.rp = static_cast<const uint8_t*>(ord[i].W);
        s.y = ord[i].y;
        s.rows = ord[i].rows;
        s.tiles = tiles[i];
        s.p2_off = (size_t)tiles[i] * nsb * 2 * rp_s1(dts[i]);
        if (s.p2_off + (size_t)tiles[i] * nsb * rp_s2(dts[i]) > 0xFFFFFFF0ull) return NTK_E_SHAPE;   // (32-bit item offsets)
        if (silu_pair && i == 1) { const RpSeg& g0 = p.seg[0]; s.wg0 = g0.wg0; s.nwg = g0.nwg; s.kb = g0.kb; s.krem = g0.krem; continue; }
        s.wg0 = wg; s.nwg = plan.nwg[i];
        s.kb = tiles[i] / s.nwg; s.krem = tiles[i] % s.nwg;
        wg += plan.nwg[i];
    }
    p.nseg = nseg; p.nseg_a = na;
    p.x = x; p.in = in_features; p.nsb = nsb;
    p.norm_w = norm_w; p.eps = eps; p.resid = resid; p.silu_pair = silu_pair;
    RpFn fn = nullptr;
    const bool nm = norm_w != nullptr;
    if (dta == dtb) {
        fn = dta == NTK_DT_Q4_K ? rp_fn<NTK_DT_Q4_K, NTK_DT_Q4_K>(nm) : dta == NTK_DT_Q5_K ? rp_fn<NTK_DT_Q5_K, NTK_DT_Q5_K>(nm) : rp_fn<NTK_DT_Q6_K, NTK_DT_Q6_K>(nm);
    } else if (dta == NTK_DT_Q4_K && dtb == NTK_DT_Q6_K) fn = rp_fn<NTK_DT_Q4_K, NTK_DT_Q6_K>(nm);
    else if (dta == NTK_DT_Q4_K && dtb == NTK_DT_Q5_K) fn = rp_fn<NTK_DT_Q4_K, NTK_DT_Q5_K>(nm);
    else if (dta == NTK_DT_Q6_K && dtb == NTK_DT_Q4_K) fn = rp_fn<NTK_DT_Q6_K, NTK_DT_Q4_K>(nm);
    else if (dta == NTK_DT_Q5_K && dtb == NTK_DT_Q4_K) fn = rp_fn<NTK_DT_Q5_K, NTK_DT_Q4_K>(nm);
    else return NTK_E_DTYPE;
    if (!fn) return NTK_E_LAUNCH;
#ifdef NTK_TUNE
    g_rp_last_nw = plan.nw; g_rp_last_grid = plan.grid; g_rp_last_lds = (int)plan.lds;
#endif
#ifdef NTK_GEMV_TRACE
    static int trace_counter = 0;
    p.trace_slot = trace_counter++;
#endif
    hipLaunchKernelGGL(fn, dim3((unsigned)plan.grid), dim3((unsigned)(64 * plan.nw)), plan.lds, resolve_stream(stream), p);
    return last_launch_status();
}

int ntk_gemv_rp(float* y, const void* rp, const float* x, int out_features, int in_features, int weight_dtype, void* stream) {
    if (!ntk::rp_supported(weight_dtype)) return NTK_E_DTYPE;   // the 1:1 form is the matrix-core GEMV: K-quants (Q8_0 rows go through the fused entry point)
    ntk_gemv_seg seg{rp, y, out_features, weight_dtype};
    return ntk_gemv_rp_fused(&seg, 1, x, in_features, nullptr, 0.0f, nullptr, 0, stream);
}

#ifdef NTK_TUNE
// tuning builds (make tune): waves per workgroup / workgroups per CU of every rp launch, 0 = the planner's choice
NTK_EXTRA_API void ntk_tune_rp_plan(int nw, int per_cu) { ntk::g_rp_force_nw = nw; ntk::g_rp_force_per_cu = per_cu; }
NTK_EXTRA_API void ntk_tune_rp_waves(int nw) { ntk_tune_rp_plan(nw, 0); }
NTK_EXTRA_API void ntk_tune_rp_last_plan(int* out3) { out3[0] = ntk::g_rp_last_nw; out3[1] = ntk::g_rp_last_grid; out3[2] = ntk::g_rp_last_lds; }
#endif

#ifdef NTK_GEMV_TRACE
NTK_EXTRA_API int ntk_debug_rp_trace(unsigned long long* out, size_t n) {   // n <= RT_SLOTS * RT_WG * RT_EV
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ntk::g_rp_trace), n * sizeof(unsigned long long)) == hipSuccess ? 0 : -3;
}
#endif

int ntk_debug_rp_prologue(uint8_t* out, const float* x, const float* norm_w, float eps, int in_features, int nsub, int nwaves, void* stream) {
    if (!out || !x) return NTK_E_NULL;
    if (in_features <= 0 || in_features % 256 != 0 || (nsub != 8 && nsub != 16) || nwaves < 1 || nwaves > 16) return NTK_E_SHAPE;
    const int nsb = in_features / 256;
    const size_t lds = ntk::rp_lds_bytes(in_features, nsb, nwaves, 1);
    if (lds > 160 * 1024) return NTK_E_SHAPE;
    using Fn = void (*)(uint8_t*, const float*, const float*, float, int, int);
    Fn fn = nsub == 8 ? (norm_w ? ntk::rp_prologue_dump_kernel<8, true> : ntk::rp_prologue_dump_kernel<8, false>)
                      : (norm_w ? ntk::rp_prologue_dump_kernel<16, true> : ntk::rp_prologue_dump_kernel<16, false>);
    if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) return NTK_E_LAUNCH;
    hipLaunchKernelGGL(fn, dim3(1), dim3((unsigned)(64 * nwaves)), lds, ntk::resolve_stream(stream), out, x, norm_w, eps, in_features, nsb);
    return ntk::last_launch_status();
}

int ntk_debug_mfma_i8_probe(int* D, const int8_t* A, const int8_t* B, void* stream) {
    if (!D || !A || !B) return NTK_E_NULL;
    hipLaunchKernelGGL(ntk::rp_mfma_probe_kernel, dim3(1), dim3(64), 0, ntk::resolve_stream(stream), D, A, B);
    return ntk::last_launch_status();
}

}  // extern "C"
