// gemm_f16.hip -- batched prompt projections on the FP16 matrix cores, 64 tokens per pass over the weights.
//
// Replaces the reference's prefill, which runs launch_gemv once per prompt token and matrix
// (reference src/model/attention.cpp:144-162,200-210, src/model/ffn.cpp:96-133), and supersedes gemm_prefill.hip's F32-MFMA
// form (16 tokens per pass, 29-65 TFLOP/s of the 157 TFLOP/s F32 matrix rate) for the formats of the target models.
//
// Arithmetic -- exact products, F32 accumulation, activations within one F32 ulp of the reference's:
//   * a GGUF weight is (integer) x (scale): the INTEGER part (Q8_0: -128..127, Q4_K: 0..15, Q6_K: -32..31) is exact in FP16;
//   * an F32 activation x is scaled by a power of two s -- one per token, chosen so that the token's largest |x| s lies in
//     [2^14, 2^15) -- and split into TWO FP16 pieces: h1 = rn16(x s), h2 = rn16(x s - h1).  The difference is exact in F32 (13
//     significant bits), so |x s - h1 - h2| <= 2^-23 |x s| -- one F32 ulp of the activation -- for every x within 2^-16 of the
//     token's largest, and <= 2^-25 / s (2^-39 of the largest) below that, where h2 is an FP16 subnormal (2^-28 of the largest if
//     the matrix cores flush it) -- against the 2^-24 every F32 addition of the reference's own accumulation (gemm.cu:129-141)
//     rounds by.  Round 2 used three BF16 pieces (8 + 8 + 8 bits, nothing rounded at all): one third more matrix instructions
//     and operand traffic for that last ulp;
//   * sum_k q_k x_k over a 32-column block = two v_mfma_f32_16x16x32_f16 whose FP16 x FP16 products are exact in the F32
//     accumulator; the per-block scale (FP16 d, 6-bit K-quant sub-scales, Q6_K's int8 sub-scales per 16 columns) multiplies
//     the F32 block sum afterwards and 1 / s the finished sum (powers of two: exact) -- the same factorisation as reference
//     gemm.cu:129-141, 190-244, 421-459;
//   * the K-quant minimum -dmin sum_j m_j S_j (S_j = sum_k (x s)_k of sub-block j) is a K = 8 product per super-block: the
//     6-bit m_j exact in FP16, S_j / 64 as two FP16 pieces (the same <= 2^-23 relative rounding), two MFMAs per tile and
//     super-block and one FMA with -64 dmin.
//
// Decomposition (gfx950, wave64):
//   * pre-pass (row_scale_kernel, split_x_kernel): the tokens' scales; X[T,in] F32 -> two FP16 planes in MFMA operand order,
//     1 KiB per (32-column step, plane, 16-token block), plus per (step, token) the sum of x s as two FP16 pieces (K-quant
//     minimum); written once per distinct X, read from L2 by every workgroup;
//   * main kernel: workgroup = 4 waves, wave = 16*RT output rows x 64 (or, grid permitting, 128) tokens (RT*4 or RT*8
//     accumulator tiles of 16x16); the operand planes of a step (8 KB per 64 tokens) reach an LDS ring of 3-8 slots by LDS-DMA
//     with exact explicit waits; the raw GGUF rows travel HBM -> registers (inline-asm loads: see the ring below) -> a per-wave
//     LDS image in units of whole blocks and become FP16 integers in two stages, two steps and one step ahead of their MFMAs;
//   * MFMA operand slots: lane (i = lane % 16, g = lane / 16) holds columns {4g..4g+3} and {16+4g..16+4g+3} of the 32-column
//     step for row / token i -- the same permutation on both operands, so the dot product is unchanged, and the two halves are
//     the two 16-column sub-scale groups of Q6_K (which uses two K = 16 MFMAs per step).
// Bound: instruction issue (MFMA + VALU of two waves per SIMD) under a 1.65-1.7 GHz clock; matrix pipe 41 % busy.
#include "common.hip.h"
#include <algorithm>
#include <cstdlib>
#include <type_traits>
#include "gemm_f16_plan.h"

namespace ntk {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// bytes k, k + 1 of a dword -> an FP16 pair, one SDWA conversion each (through F32 it is two conversions and a pack per pair: the
// VALU slots of a step are what the kernel runs out of first); `s_nop 1`: see cvt8_s8_f16 below (these feed the minimum term's matrix instruction)
template <int K> __device__ __forceinline__ uint32_t cvt2_s8_f16(uint32_t q) {
    uint32_t r;
    if constexpr (K == 0)
        asm("v_cvt_f16_i16_sdwa %0, sext(%1) dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:BYTE_0\n\t"
            "v_cvt_f16_i16_sdwa %0, sext(%1) dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1\n\ts_nop 1" : "=&v"(r) : "v"(q));
    else
        asm("v_cvt_f16_i16_sdwa %0, sext(%1) dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:BYTE_2\n\t"
            "v_cvt_f16_i16_sdwa %0, sext(%1) dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_3\n\ts_nop 1" : "=&v"(r) : "v"(q));
    return r;
}
template <int K> __device__ __forceinline__ uint32_t cvt2_u8_f16(uint32_t q) {
    uint32_t r;
    if constexpr (K == 0)
        asm("v_cvt_f16_u16_sdwa %0, %1 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:BYTE_0\n\t"
            "v_cvt_f16_u16_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1\n\ts_nop 1" : "=&v"(r) : "v"(q));
    else
        asm("v_cvt_f16_u16_sdwa %0, %1 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:BYTE_2\n\t"
            "v_cvt_f16_u16_sdwa %0, %1 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_3\n\ts_nop 1" : "=&v"(r) : "v"(q));
    return r;
}
// Eight bytes -> the 8 FP16 integers of an MFMA operand, ONE asm statement that ends in `s_nop 1`: a matrix instruction may read a VGPR two wait states
// after a VALU wrote it, hipcc pads an asm statement it cannot see into with ONE (the guide's "just-written v operand -> MFMA operand" row), and whether
// anything else stood between the conversion and the MFMA was up to the scheduler -- round 6's K-slice kernel came out with `;;#ASMEND, s_nop 0, v_mfma`
// in some builds: whole tiles wrong, differently from launch to launch (profiles/r06_prompt_kslice.txt).
__device__ __forceinline__ u32x4 cvt8_s8_f16(uint32_t lo, uint32_t hi) {
    uint32_t r0, r1, r2, r3;
    asm("v_cvt_f16_i16_sdwa %0, sext(%4) dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:BYTE_0\n\t"
        "v_cvt_f16_i16_sdwa %0, sext(%4) dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1\n\t"
        "v_cvt_f16_i16_sdwa %1, sext(%4) dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:BYTE_2\n\t"
        "v_cvt_f16_i16_sdwa %1, sext(%4) dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_3\n\t"
        "v_cvt_f16_i16_sdwa %2, sext(%5) dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:BYTE_0\n\t"
        "v_cvt_f16_i16_sdwa %2, sext(%5) dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1\n\t"
        "v_cvt_f16_i16_sdwa %3, sext(%5) dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:BYTE_2\n\t"
        "v_cvt_f16_i16_sdwa %3, sext(%5) dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_3\n\t"
        "s_nop 1" : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(lo), "v"(hi));
    return u32x4{r0, r1, r2, r3};
}
__device__ __forceinline__ u32x4 cvt8_u8_f16(uint32_t lo, uint32_t hi) {
    uint32_t r0, r1, r2, r3;
    asm("v_cvt_f16_u16_sdwa %0, %4 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:BYTE_0\n\t"
        "v_cvt_f16_u16_sdwa %0, %4 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1\n\t"
        "v_cvt_f16_u16_sdwa %1, %4 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:BYTE_2\n\t"
        "v_cvt_f16_u16_sdwa %1, %4 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_3\n\t"
        "v_cvt_f16_u16_sdwa %2, %5 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:BYTE_0\n\t"
        "v_cvt_f16_u16_sdwa %2, %5 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_1\n\t"
        "v_cvt_f16_u16_sdwa %3, %5 dst_sel:WORD_0 dst_unused:UNUSED_PAD src0_sel:BYTE_2\n\t"
        "v_cvt_f16_u16_sdwa %3, %5 dst_sel:WORD_1 dst_unused:UNUSED_PRESERVE src0_sel:BYTE_3\n\t"
        "s_nop 1" : "=&v"(r0), "=&v"(r1), "=&v"(r2), "=&v"(r3) : "v"(lo), "v"(hi));
    return u32x4{r0, r1, r2, r3};
}
typedef uint32_t __attribute__((aligned(2))) u32_a2;
typedef uint16_t __attribute__((aligned(2))) u16_a2;

// ---- pre-pass 1: the tokens' scales --------------------------------------------------------------------------------------------
// s = 2^(14 - floor(log2 m)), m = the token's largest |x|: m s in [2^14, 2^15) -- FP16's largest binade but one.  Exponent fields are
// kept inside [1, 253] so that both s and 1 / s are normal numbers (an all-zero or subnormal token multiplies to zero either way; a
// token holding Inf / NaN propagates it through the first piece).  grid = ceil(T / 4), block = 256: one wave per token.
// exponent field of s from the token's largest |x| (bit pattern; a NaN pattern counts as the largest binade: any scale will do then)
__device__ __forceinline__ int scale_exp_of_max(uint32_t max_bits) {
    const int em = (int)((max_bits >> 23) & 0xFFu);
    return min(253, max(1, 268 - em));
}
__global__ __launch_bounds__(256) void row_scale_kernel(const float* __restrict__ X, int T, int in, float* __restrict__ scale, float* __restrict__ inv) {
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= T) return;
    const float4* row = reinterpret_cast<const float4*>(X + (size_t)t * in);
    float m = 0.0f;
    for (int c = lane; c < in / 4; c += 64) {
        const float4 v = row[c];
        m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    uint32_t mb = __float_as_uint(m);
    if (m != m) mb = 0x7F800000u;   // (fmaxf drops NaNs: a NaN anywhere in the row is found by the planes, any scale will do)
    const int es = scale_exp_of_max(mb);
    if (lane == 0) {
        scale[t] = __uint_as_float((uint32_t)es << 23);
        inv[t] = __uint_as_float((uint32_t)(254 - es) << 23);
    }
}

// ---- pre-pass 2: X -> FP16 planes in operand order + per-step sums ---------------------------------------------------------------
// grid = (in / 32 steps + 8 (a record of zeros and a whole unit of zero sums), 64-token chunks), block = 256 = 4 token blocks x 64 lanes
// FROM_MAX: `scale` holds the tokens' largest |x| (written by the kernel that PRODUCED X: rmsnorm_rowmax_kernel, silu_mul_rowmax_kernel below) instead
// of their scales -- no row_scale_kernel pass over X; the blocks of step 0 leave 1 / s in `inv` for the main kernel
template <bool FROM_MAX>
__global__ __launch_bounds__(256) void split_x_kernel(const float* __restrict__ X, int T, int in, u32x4* __restrict__ xb, float* __restrict__ aux,
                                                      size_t chunk_bytes, const float* __restrict__ scale, float* __restrict__ inv) {
    const int step = blockIdx.x, tb = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4, t = tb * 16 + j;
    // blockIdx.y = 64-token chunk: its tokens, its planes
    X += (size_t)blockIdx.y * GB_TOK * in;
    scale += (size_t)blockIdx.y * GB_TOK;
    if constexpr (FROM_MAX) inv += (size_t)blockIdx.y * GB_TOK;
    T = min(GB_TOK, T - (int)blockIdx.y * GB_TOK);
    xb = reinterpret_cast<u32x4*>(reinterpret_cast<uint8_t*>(xb) + blockIdx.y * chunk_bytes);
    aux = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(aux) + blockIdx.y * chunk_bytes);
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = 0.0f;
    float sc = 1.0f;
    if (t < T && step * 32 < in) {   // block in/32 writes the all-zero record that K ranges rounded up to whole trips read
        const float* row = X + (size_t)t * in + step * 32 + 4 * g;
        const float4 a = *reinterpret_cast<const float4*>(row), b = *reinterpret_cast<const float4*>(row + 16);
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        if constexpr (FROM_MAX) {
            const int es = scale_exp_of_max(__float_as_uint(scale[t]));
            sc = __uint_as_float((uint32_t)es << 23);
            if (step == 0 && g == 0) inv[t] = __uint_as_float((uint32_t)(254 - es) << 23);
        } else {
            sc = scale[t];
        }
    }
    float p1[8], p2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {   // h1 = rn16(x s); the remainder is exact in F32 (13 significant bits) and h2 = rn16(remainder)
        x[e] *= sc;
        const _Float16 h1 = (_Float16)x[e];
        p1[e] = (float)h1;
        p2[e] = x[e] - p1[e];
    }
    auto pk = [](float lo, float hi) {   // round-to-nearest conversions (p1 is already an FP16 value: exact)
        const f16x2 h = {(_Float16)lo, (_Float16)hi};
        return __builtin_bit_cast(uint32_t, h);
    };
    if (step * 32 <= in) {   // (blocks in/32 + 1 .. in/32 + 7 only complete the all-zero unit of the sums below)
        const size_t base = ((size_t)step * GB_PLANES * 4 + tb) * 64 + lane;   // plane p at + p * 4 * 64
        xb[base] = u32x4{pk(p1[0], p1[1]), pk(p1[2], p1[3]), pk(p1[4], p1[5]), pk(p1[6], p1[7])};
        xb[base + 256] = u32x4{pk(p2[0], p2[1]), pk(p2[2], p2[3]), pk(p2[4], p2[5]), pk(p2[6], p2[7])};
    }
    // sum of the step's 32 scaled activations of token t (fixed order: the lane's 8 in sequence, then the 4 column groups), as two FP16
    // pieces of sum / 64 (|sum| <= 32 * 2^15) in the operand layout of the K-quant minimum MFMA: per unit of 8 steps a 2 KB record
    // [piece][token block][step / 4][token] x (4 steps x FP16) -- lane (token, g < 2) of that MFMA reads its 8 bytes in one piece
    float sum = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    if (g == 0) {
        const float y = sum * 0.015625f;
        const _Float16 h1 = (_Float16)y, h2 = (_Float16)(y - (float)h1);
        _Float16* rec = reinterpret_cast<_Float16*>(reinterpret_cast<uint8_t*>(aux) + (size_t)(step >> 3) * GB_MIN_UNIT_BYTES);
        const int pos = ((tb * 2 + ((step >> 2) & 1)) * 64 + j * 4 + (step & 3));   // in FP16 units, piece 0; piece 1 at + 4 * 128
        rec[pos] = h1;
        rec[4 * 128 + pos] = h2;
    }
}

// ---- producers that leave the tokens' largest |x| beside X (so that the pre-pass above needs no pass of its own over X) ----------
// RMSNorm (elementwise.hip's rmsnorm_kernel, reference rmsnorm.cu:60-68, same expressions) + max |y| per token; zero (optional): T floats set to
// 0 for a LATER launch that accumulates maxima with atomics (silu_mul_rowmax_kernel).  One workgroup per token.
__global__ __launch_bounds__(1024) void rmsnorm_rowmax_kernel(float* __restrict__ output, const float* __restrict__ input, const float* __restrict__ weight,
                                                              int hidden, float eps, float* __restrict__ row_max, float* __restrict__ zero) {
    __shared__ float red[16];
    const float* x = input + (size_t)blockIdx.x * hidden;
    float ssq = 0.0f;
    for (int i = threadIdx.x; i < hidden; i += blockDim.x) ssq = fmaf(x[i], x[i], ssq);
    const float tot = block_sum(ssq, red);
    const float rms_inv = 1.0f / sqrtf(tot / (float)hidden + eps);
    uint32_t mb = 0;   // (bit patterns of |y|: ordered like the values, and a NaN is not dropped)
    for (int i = threadIdx.x; i < hidden; i += blockDim.x) {
        const float v = x[i] * rms_inv * weight[i];
        output[(size_t)blockIdx.x * hidden + i] = v;
        mb = max(mb, __float_as_uint(v) & 0x7FFFFFFFu);
    }
    __syncthreads();   // (red is reused)
    const float m = block_max(__uint_as_float(mb <= 0x7F800000u ? mb : 0x7F800000u), red);   // (NaN -> the largest binade, like row_scale_kernel's rule)
    if (threadIdx.x == 0) {
        row_max[blockIdx.x] = m;
        if (zero) zero[blockIdx.x] = 0.0f;
    }
}
// out = silu(gate) * up (elementwise.hip's silu_mul_kernel, reference gemm.cu:719-724) + max |out| per token, accumulated with one atomic per
// workgroup on the bit pattern (non-negative floats order like their bits).  grid (ceil(I / 1024), T), 256 threads x 4 elements; I % 4 == 0.
__global__ __launch_bounds__(256) void silu_mul_rowmax_kernel(float* __restrict__ out, const float* __restrict__ gate, const float* __restrict__ up, int I,
                                                              float* __restrict__ row_max) {
    __shared__ float red[16];
    const int t = blockIdx.y, i = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
    uint32_t mb = 0;
    if (i < I) {
        const size_t at = (size_t)t * I + i;
        const float4 g = *reinterpret_cast<const float4*>(gate + at), u = *reinterpret_cast<const float4*>(up + at);
        float4 o;
        o.x = g.x / (1.0f + expf(-g.x)) * u.x; o.y = g.y / (1.0f + expf(-g.y)) * u.y;
        o.z = g.z / (1.0f + expf(-g.z)) * u.z; o.w = g.w / (1.0f + expf(-g.w)) * u.w;
        *reinterpret_cast<float4*>(out + at) = o;
        mb = max(max(__float_as_uint(o.x) & 0x7FFFFFFFu, __float_as_uint(o.y) & 0x7FFFFFFFu),
                 max(__float_as_uint(o.z) & 0x7FFFFFFFu, __float_as_uint(o.w) & 0x7FFFFFFFu));
    }
    const float m = block_max(__uint_as_float(mb <= 0x7F800000u ? mb : 0x7F800000u), red);
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned*>(row_max) + t, __float_as_uint(m));
}

// ---- the operand pre-pass INSIDE the launch that produces X (round 6, late) -------------------------------------------------------------------------
// split_x_kernel costs a launch (and, without the producers' row maxima, row_scale_kernel a second one) in front of every projection: four to five of the
// fourteen launches of a layer, a quarter of a short prompt's time.  The kernels below own a whole TOKEN per workgroup, so the workgroup that has written a
// token's row knows its largest |x| and can split the row itself: planes, step sums and 1 / s go straight into the GEMM workspace and the projection runs
// with reuse_x = 1.  split_row is split_x_kernel's arithmetic element for element (same scale, same two roundings, the step sums in the same order): the
// workspace holds the same bits.  Layout of the workspace: [chunk][(in / 32 + 1) step records of 8 KB | sums of the units], then [1 / s][s] of the pass.
// row: the token's `in` floats (global memory; written by THIS workgroup before a __syncthreads()), or null for a padding token (zeros: the records the
// matrix instructions read beside the prompt's last tokens).  Every thread of the workgroup calls it.
__device__ __forceinline__ void split_row(const float* row, uint32_t max_bits, int t, int in, uint8_t* __restrict__ ws) {
    const size_t chunk_bytes = ws_chunk_bytes(in);
    const int chunk = t / GB_TOK, tl = t - chunk * GB_TOK, tb = tl >> 4, j = tl & 15;
    u32x4* xb = reinterpret_cast<u32x4*>(ws + (size_t)chunk * chunk_bytes);
    uint8_t* aux = ws + (size_t)chunk * chunk_bytes + (size_t)(in / 32 + 1) * GB_STEP_BYTES;
    const int es = scale_exp_of_max(max_bits);
    const float sc = __uint_as_float((uint32_t)es << 23);
    if (threadIdx.x == 0) reinterpret_cast<float*>(ws + (size_t)GB_MAX_CHUNKS * chunk_bytes)[t] = __uint_as_float((uint32_t)(254 - es) << 23);   // 1 / s
    const int ngroups = (in / 32 + 8) * 4;   // (steps in / 32 .. + 7: the record of zeros and a whole unit of zero sums, as split_x_kernel's last blocks)
    for (int cg = (int)threadIdx.x; cg < ngroups; cg += (int)blockDim.x) {   // 4 consecutive lanes = the 4 column groups of a step
        const int step = cg >> 2, g = cg & 3;
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.0f;
        if (row && step * 32 < in) {
            const float* src = row + step * 32 + 4 * g;
            const float4 a = *reinterpret_cast<const float4*>(src), b = *reinterpret_cast<const float4*>(src + 16);
            x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
        }
        float p1[8], p2[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            x[e] *= sc;
            const _Float16 h1 = (_Float16)x[e];
            p1[e] = (float)h1;
            p2[e] = x[e] - p1[e];
        }
        auto pk = [](float lo, float hi) {
            const f16x2 h = {(_Float16)lo, (_Float16)hi};
            return __builtin_bit_cast(uint32_t, h);
        };
        if (step * 32 <= in) {
            const size_t base = ((size_t)step * GB_PLANES * 4 + tb) * 64 + (j + 16 * g);
            xb[base] = u32x4{pk(p1[0], p1[1]), pk(p1[2], p1[3]), pk(p1[4], p1[5]), pk(p1[6], p1[7])};
            xb[base + 256] = u32x4{pk(p2[0], p2[1]), pk(p2[2], p2[3]), pk(p2[4], p2[5]), pk(p2[6], p2[7])};
        }
        float sum = ((x[0] + x[1]) + (x[2] + x[3])) + ((x[4] + x[5]) + (x[6] + x[7]));
        sum += __shfl_xor(sum, 1, 64);   // (split_x_kernel: + column group g ^ 1, then + the other pair)
        sum += __shfl_xor(sum, 2, 64);
        if (g == 0) {
            const float y = sum * 0.015625f;
            const _Float16 h1 = (_Float16)y, h2 = (_Float16)(y - (float)h1);
            _Float16* rec = reinterpret_cast<_Float16*>(aux + (size_t)(step >> 3) * GB_MIN_UNIT_BYTES);
            const int pos = ((tb * 2 + ((step >> 2) & 1)) * 64 + j * 4 + (step & 3));
            rec[pos] = h1;
            rec[4 * 128 + pos] = h2;
        }
    }
}

// X[T][in] (any producer) -> workspace: row maximum + split, one workgroup per token (instead of row_scale_kernel + split_x_kernel)
__global__ __launch_bounds__(256) void rowmax_split_kernel(const float* __restrict__ X, int T, int in, uint8_t* __restrict__ ws) {
    __shared__ float red[16];
    const int t = (int)blockIdx.x;
    const float* row = t < T ? X + (size_t)t * in : nullptr;
    float m = 0.0f;
    if (row)
        for (int c = (int)threadIdx.x; c < in / 4; c += (int)blockDim.x) {
            const float4 v = reinterpret_cast<const float4*>(row)[c];
            m = fmaxf(fmaxf(m, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
        }
    m = block_max(m, red);   // (exact whatever the order; fmaxf drops NaNs as row_scale_kernel's does: a NaN is found by the planes)
    split_row(row, __float_as_uint(m), t, in, ws);
}
// rmsnorm_rowmax_kernel + the split of the row it has written
__global__ __launch_bounds__(1024) void rmsnorm_split_kernel(float* __restrict__ output, const float* __restrict__ input, const float* __restrict__ weight,
                                                             int T, int hidden, float eps, uint8_t* __restrict__ ws) {
    __shared__ float red[16];
    const int t = (int)blockIdx.x;
    if (t >= T) { split_row(nullptr, 0u, t, hidden, ws); return; }   // (uniform per workgroup)
    const float* x = input + (size_t)t * hidden;
    float* out = output + (size_t)t * hidden;
    float ssq = 0.0f;
    for (int i = threadIdx.x; i < hidden; i += blockDim.x) ssq = fmaf(x[i], x[i], ssq);
    const float tot = block_sum(ssq, red);
    const float rms_inv = 1.0f / sqrtf(tot / (float)hidden + eps);
    uint32_t mb = 0;
    for (int i = threadIdx.x; i < hidden; i += blockDim.x) {
        const float v = x[i] * rms_inv * weight[i];
        out[i] = v;
        mb = max(mb, __float_as_uint(v) & 0x7FFFFFFFu);
    }
    __syncthreads();   // (red is reused; the row is written)
    const float m = block_max(__uint_as_float(mb <= 0x7F800000u ? mb : 0x7F800000u), red);
    __syncthreads();   // (workgroup-scope: every thread's stores to `out` are visible to the threads that split them)
    split_row(out, __float_as_uint(m), t, hidden, ws);
}

// ---- per-format weight operand ---------------------------------------------------------------------------------------------
// The raw GGUF rows travel HBM -> registers -> a per-wave LDS image in UNITS of whole blocks (Q8_0: 4 blocks = 136 B, K-quants:
// one 256-column super-block), as 16-byte pieces of the 16-byte-aligned window that covers the unit: 16 bytes per lane and
// NCH consecutive lanes per row, i.e. >= 144 contiguous bytes per row and request (a lane-per-slot gather of 4-byte pieces,
// 16 bytes per row and request, tops out near 2.4 TB/s in the address coalescer).  Each 32-column step then reads its slot
// (row i, columns {4g..4g+3, 16+4g..16+4g+3}) out of the image with 2-byte-aligned LDS dword reads.  STRIDE (bytes between row
// images) = 4 x an odd number of dwords... chosen so that the 16 rows x 4 column groups of one read hit 64 different banks.
struct AOp {
    u32x4 a;            // 8 FP16 integers
    float s0, s1;       // scale of the slot's low / high 4 columns (equal unless the format scales per 16 columns)
};
template <bool AL> __device__ __forceinline__ uint32_t lds32(const uint8_t* p) {   // LDS dword: 4-byte aligned (AL) or 2-byte aligned (slow)
    if constexpr (AL) return *reinterpret_cast<const uint32_t*>(p);
    else return *reinterpret_cast<const u32_a2*>(p);
}
__device__ __forceinline__ uint32_t lds16(const uint8_t* p) { return *reinterpret_cast<const u16_a2*>(p); }
// bytes [2, 6) of the 8 bytes (lo, hi): the dword that sits 2 bytes past a 4-byte boundary.  (A misaligned ds_read_b32 works and
// costs several hundred cycles per wave-instruction -- the step timeline of round 3, profiles/r03_prompt_gemm_f16.txt -- so
// every LDS dword read of the decoders is aligned and the misaligned ones are two aligned dwords + one v_alignbyte.)
__device__ __forceinline__ uint32_t mid32(uint32_t lo, uint32_t hi) { return __builtin_amdgcn_alignbyte(hi, lo, 2u); }
template <int DT> struct DeqI;

// A step's weight operand is made in two stages one step apart, so that no VALU instruction inside a step's MFMA chain waits for an
// LDS read of the same step: load() -- the slot's raw dwords out of the wave's image (and whatever needs the unit's header, which
// changes a step before the unit's last operand is converted) -- runs two steps ahead of the MFMAs, convert() one step ahead.
// j = step within the unit, k = parity of the unit (both compile-time after unrolling).  row = the row's image + the unit's
// shift (4-byte aligned: the launch checks the row pitch), rowg = row + 4 g.

template <> struct DeqI<NTK_DT_Q8_0> : GemmFmt<NTK_DT_Q8_0> {   // types.h:104-108: half d, int8 qs[32]
    static constexpr int UB = 136, NCH = 10;                          // unit = 4 blocks; window: shift (0, 4, 8 or 12) + 136 <= 160 (< STRIDE = 176)
    static constexpr int NRING = GB_NRING_Q8;                         // units in flight per wave (register ring): 8 steps ahead of the MFMAs
    static constexpr int PPI = 0;
    struct Hdr {};
    struct MinOp {};
    __device__ static MinOp min_operand(const Hdr&, int) { return MinOp{}; }
    struct Raw { uint32_t w0, w1, w2, w3, d; };
    __device__ static Hdr header(const uint8_t*, const uint8_t*) { return Hdr{}; }
    template <bool AL> __device__ static Raw load(const uint8_t* row, const uint8_t* rowg, const Hdr&, int j, int) {
        Raw r;   // the block's quants start 34 j + 2 bytes into the unit: on a dword boundary for odd j, 2 bytes past one for even j
        if (!AL || (j & 1)) { r.w0 = lds32<AL>(rowg + 34 * j + 2); r.w2 = lds32<AL>(rowg + 34 * j + 18); r.w1 = r.w3 = 0; }
        else { r.w0 = lds32<AL>(rowg + 34 * j); r.w1 = lds32<AL>(rowg + 34 * j + 4); r.w2 = lds32<AL>(rowg + 34 * j + 16); r.w3 = lds32<AL>(rowg + 34 * j + 20); }
        r.d = lds16(row + 34 * j);
        return r;
    }
    template <bool AL> __device__ static AOp convert(const Raw& r, int j, int) {
        const bool whole = !AL || (j & 1);
        const uint32_t lo = whole ? r.w0 : mid32(r.w0, r.w1), hi = whole ? r.w2 : mid32(r.w2, r.w3);
        AOp o;
        o.a = cvt8_s8_f16(lo, hi);
        o.s0 = o.s1 = h2f((uint16_t)r.d);
        return o;
    }
};

template <> struct DeqI<NTK_DT_Q4_0> : GemmFmt<NTK_DT_Q4_0> {   // types.h:97-100: half d, 16 bytes of nibbles: w_j = d (lo_j - 8), w_{j+16} = d (hi_j - 8)  (gemm.cu:32-86)
    static constexpr int UB = 144, NCH = 10;                          // unit = 8 blocks; window: shift (<= 14) + 144 <= 160 (< STRIDE = 176)
    static constexpr int NRING = 1, PPI = 0;
    struct Hdr {};
    struct MinOp {};
    __device__ static MinOp min_operand(const Hdr&, int) { return MinOp{}; }
    struct Raw { uint32_t w0, w1, d; };
    __device__ static Hdr header(const uint8_t*, const uint8_t*) { return Hdr{}; }
    // the lane's columns {4g..4g+3} and {16+4g..16+4g+3} are the low and high nibbles of the SAME four bytes: one dword per step, 2 bytes
    // past a dword boundary for even j (18 j + 2), on one for odd j
    template <bool AL> __device__ static Raw load(const uint8_t* row, const uint8_t* rowg, const Hdr&, int j, int) {
        Raw r;
        if (!AL || (j & 1)) { r.w0 = lds32<AL>(rowg + 18 * j + 2); r.w1 = 0; }
        else { r.w0 = lds32<AL>(rowg + 18 * j); r.w1 = lds32<AL>(rowg + 18 * j + 4); }
        r.d = lds16(row + 18 * j);
        return r;
    }
    template <bool AL> __device__ static AOp convert(const Raw& r, int j, int) {
        const uint32_t q = (!AL || (j & 1)) ? r.w0 : mid32(r.w0, r.w1);
        const u32x4 qa = cvt8_u8_f16(q & 0x0F0F0F0Fu, (q >> 4) & 0x0F0F0F0Fu);
        const f16x2 m8 = {(_Float16)-8.0f, (_Float16)-8.0f};
        auto sub8 = [&](uint32_t w) { return __builtin_bit_cast(uint32_t, (f16x2)(__builtin_bit_cast(f16x2, w) + m8)); };
        AOp o;   // n - 8: exact small integers
        o.a = u32x4{sub8(qa.x), sub8(qa.y), sub8(qa.z), sub8(qa.w)};
        o.s0 = o.s1 = h2f((uint16_t)r.d);
        return o;
    }
};

template <> struct DeqI<NTK_DT_Q4_K> : GemmFmt<NTK_DT_Q4_K> {   // types.h:112-117: half d, dmin; 12 packed 6-bit (scale, min); 128 bytes of nibbles
    static constexpr int UB = 144, NCH = 9;                            // rows are 16-byte aligned: no shift (STRIDE = UB)
    static constexpr int NRING = 1, PPI = 0;
    struct Hdr { u32x4 h; };   // d | dmin, 12 scale bytes
    // the unit's 8 minima as the weight-side operand of the minimum-term MFMA: lane group g < 2 holds m_{4g} .. m_{4g+3} (FP16, exact),
    // the others zeros; -64 dmin for the FMA behind it (the sums are stored divided by 64)   (6-bit packing: gemm.cu:206-222)
    struct MinOp { uint32_t m0, m1; float ndmin64; };
    template <typename H> __device__ static MinOp min_operand(const H& hd, int g) {
        const uint32_t w0 = hd.h.z & 0x3F3F3F3Fu;
        const uint32_t w1 = ((hd.h.w >> 4) & 0x0F0F0F0Fu) | (((hd.h.z >> 6) & 0x03030303u) << 4);
        const uint32_t w = g == 0 ? w0 : (g == 1 ? w1 : 0u);
        return MinOp{cvt2_u8_f16<0>(w), cvt2_u8_f16<2>(w), -64.0f * h2f((uint16_t)(hd.h.x >> 16))};
    }
    struct Raw { uint32_t lo, hi; float s0; };
    __device__ static Hdr header(const uint8_t* row, const uint8_t*) { return Hdr{*reinterpret_cast<const u32x4*>(row)}; }
    template <bool AL> __device__ static Raw load(const uint8_t*, const uint8_t* rowg, const Hdr& hd, int j, int) {
        float sc, mn;   // (the minima go through min_operand() once per unit)
        kq_scale_min(hd.h.y, hd.h.z, hd.h.w, j, sc, mn);                       // gemm.cu:206-222
        const float d = h2f((uint16_t)(hd.h.x & 0xFFFFu));
        return Raw{lds32<true>(rowg + 16 + 32 * (j >> 1)), lds32<true>(rowg + 32 + 32 * (j >> 1)), d * sc};
    }
    template <bool AL> __device__ static AOp convert(const Raw& r, int j, int) {
        const int sh = 4 * (j & 1);                                           // even sub-block: low nibbles, odd: high
        const uint32_t lo = (r.lo >> sh) & 0x0F0F0F0Fu, hi = (r.hi >> sh) & 0x0F0F0F0Fu;
        AOp o;
        o.a = cvt8_u8_f16(lo, hi);
        o.s0 = o.s1 = r.s0;
        return o;
    }
};

template <> struct DeqI<NTK_DT_Q5_K> : GemmFmt<NTK_DT_Q5_K> {   // types.h:122-128: half d, dmin; 12 packed 6-bit (scale, min); qh[32]; ql[128]
    static constexpr int UB = 176, NCH = 11;                           // rows are 16-byte aligned: no shift (STRIDE = UB)
    static constexpr int NRING = 1, PPI = 0;
    struct Hdr { u32x4 h; uint32_t qh_lo, qh_hi; };   // d | dmin, 12 scale bytes; the lane's 8 bytes of fifth bits (all 8 steps)
    // the unit's 8 minima as the weight-side operand of the minimum-term MFMA: lane group g < 2 holds m_{4g} .. m_{4g+3} (FP16, exact),
    // the others zeros; -64 dmin for the FMA behind it (the sums are stored divided by 64)   (6-bit packing: gemm.cu:206-222)
    struct MinOp { uint32_t m0, m1; float ndmin64; };
    template <typename H> __device__ static MinOp min_operand(const H& hd, int g) {
        const uint32_t w0 = hd.h.z & 0x3F3F3F3Fu;
        const uint32_t w1 = ((hd.h.w >> 4) & 0x0F0F0F0Fu) | (((hd.h.z >> 6) & 0x03030303u) << 4);
        const uint32_t w = g == 0 ? w0 : (g == 1 ? w1 : 0u);
        return MinOp{cvt2_u8_f16<0>(w), cvt2_u8_f16<2>(w), -64.0f * h2f((uint16_t)(hd.h.x >> 16))};
    }
    struct Raw { uint32_t lo, hi, b5lo, b5hi; float s0; };
    __device__ static Hdr header(const uint8_t* row, const uint8_t* rowg) { return Hdr{*reinterpret_cast<const u32x4*>(row), lds32<true>(rowg + 16), lds32<true>(rowg + 32)}; }
    template <bool AL> __device__ static Raw load(const uint8_t*, const uint8_t* rowg, const Hdr& hd, int j, int) {
        float sc, mn;   // (the minima go through min_operand() once per unit)
        kq_scale_min(hd.h.y, hd.h.z, hd.h.w, j, sc, mn);                       // gemm.cu:206-222 (same packing as Q4_K)
        const float d = h2f((uint16_t)(hd.h.x & 0xFFFFu));
        // fifth bit of column l of sub-block j: bit j of qh[l]   (gemm.cu:297-354: u1 = 1 << 2c, u2 = 2 << 2c)
        return Raw{lds32<true>(rowg + 48 + 32 * (j >> 1)), lds32<true>(rowg + 64 + 32 * (j >> 1)), ((hd.qh_lo >> j) & 0x01010101u) << 4, ((hd.qh_hi >> j) & 0x01010101u) << 4,
                   d * sc};
    }
    template <bool AL> __device__ static AOp convert(const Raw& r, int j, int) {
        const int sh = 4 * (j & 1);                                           // even sub-block: low nibbles, odd: high
        const uint32_t lo = ((r.lo >> sh) & 0x0F0F0F0Fu) | r.b5lo, hi = ((r.hi >> sh) & 0x0F0F0F0Fu) | r.b5hi;
        AOp o;
        o.a = cvt8_u8_f16(lo, hi);
        o.s0 = o.s1 = r.s0;
        return o;
    }
};

template <> struct DeqI<NTK_DT_Q6_K> : GemmFmt<NTK_DT_Q6_K> {   // types.h:132-137: ql[128], qh[64], int8 scales[16], half d
    static constexpr int UB = 210, NCH = 14;                           // window: shift (even, <= 14) + 210 <= 224 (< STRIDE = 240)
    static constexpr int NRING = 1, PPI = 0;
    struct Hdr { float d; };
    struct MinOp {};
    __device__ static MinOp min_operand(const Hdr&, int) { return MinOp{}; }
    struct Raw { uint32_t ql0, ql1, ql2, ql3, qh0, qh1, qh2, qh3, sc; float d; };
    __device__ static Hdr header(const uint8_t* row, const uint8_t*) { return Hdr{h2f((uint16_t)lds16(row + 208))}; }
    // blocks are 210 bytes: with a 4-byte aligned row, the units of even parity start on a dword boundary and those of odd
    // parity 2 bytes past one (k = the unit's parity: K ranges start at even units) -- `row` is the 4-byte aligned address at or
    // 2 bytes below the unit's first byte
    // (!AL: any row pitch -- `row` is the unit's first byte and the dword reads are 2-byte aligned)
    template <bool AL> __device__ static Raw load(const uint8_t* row, const uint8_t* rowg, const Hdr& hd, int j, int k) {
        if (!AL) k = 0;
        const int hf = j >> 2, t = j & 3;
        const uint8_t* ql = rowg + 64 * hf + 32 * (t & 1);
        const uint8_t* qh = rowg + 128 + 32 * hf;
        Raw r;
        r.ql0 = lds32<AL>(ql); r.ql2 = lds32<AL>(ql + 16); r.qh0 = lds32<AL>(qh); r.qh2 = lds32<AL>(qh + 16);
        if (k) { r.ql1 = lds32<AL>(ql + 4); r.ql3 = lds32<AL>(ql + 20); r.qh1 = lds32<AL>(qh + 4); r.qh3 = lds32<AL>(qh + 20); }
        else r.ql1 = r.ql3 = r.qh1 = r.qh3 = 0;
        r.sc = lds16(row + 2 * k + 192 + 8 * hf + 2 * t);   // the two int8 sub-scales of the step's 16-column halves
        r.d = hd.d;
        return r;
    }
    template <bool AL> __device__ static AOp convert(const Raw& r, int j, int k) {
        if (!AL) k = 0;
        const int t = j & 3;
        const int sl = 4 * (t >> 1), sh = 2 * t;
        const uint32_t ql_lo = k ? mid32(r.ql0, r.ql1) : r.ql0, ql_hi = k ? mid32(r.ql2, r.ql3) : r.ql2;
        const uint32_t qh_lo = k ? mid32(r.qh0, r.qh1) : r.qh0, qh_hi = k ? mid32(r.qh2, r.qh3) : r.qh2;
        const uint32_t lo = ((ql_lo >> sl) & 0x0F0F0F0Fu) | (((qh_lo >> sh) & 0x03030303u) << 4);         // gemm.cu:421-459
        const uint32_t hi = ((ql_hi >> sl) & 0x0F0F0F0Fu) | (((qh_hi >> sh) & 0x03030303u) << 4);
        AOp o;   // q - 32: exact small integers
        const u32x4 qa = cvt8_u8_f16(lo, hi);
        const f16x2 m32 = {(_Float16)-32.0f, (_Float16)-32.0f};
        auto sub32 = [&](uint32_t w) { return __builtin_bit_cast(uint32_t, (f16x2)(__builtin_bit_cast(f16x2, w) + m32)); };
        o.a = u32x4{sub32(qa.x), sub32(qa.y), sub32(qa.z), sub32(qa.w)};
        o.s0 = r.d * (float)(int)(int8_t)(r.sc & 0xFF);
        o.s1 = r.d * (float)(int)(int8_t)(r.sc >> 8);
        return o;
    }
};

// ---- the same three K-quant formats read from the ENGINE'S DECODE REPACK (csrc/gemv_rp.hip: tiles of 16 rows x 256-column super-blocks; round 6) ----
// With one resident copy of a K-quant matrix (the uploaded GGUF bytes freed after the load-time repack) the prompt GEMM used to get the tensor unpacked
// into a scratch in front of every launch (ntk_rp_unpack: -1.4 ... -8 % of a 1024-token pass, a fixed 4 ms of an 8B pass).  These decoders read the repack
// itself: the same integers and the same scale products as the raw decoders above, operand slot for operand slot -- identical bits.  A unit = the ITEM of a
// tile (two 1 KiB nibble planes P1 [+ the fifth / fifth-and-sixth bits], the rows' records P2), copied into the wave's image as it lies: lane (i, g) then
// finds the nibbles of its columns {32 j + 4 g ..+3} and {32 j + 16 + 4 g ..+3} of row i as ONE aligned dword each, 256 consecutive bytes per wave read
// (no bank conflicts, no 2-byte-aligned reads), and the sub-block scales / minima as plain bytes of the row record.
//   column c of the super-block: step s = c >> 7, half h = (c >> 6) & 1 (low / high nibble), lane group kg = (c >> 4) & 3, byte b = c & 15 of lane 16 kg + i's chunk
//   => sub-block j: s = j >> 2, h = (j >> 1) & 1, the two 16-column groups kg = 2 (j & 1) and 2 (j & 1) + 1
// `row` = the tile's image + 16 i, `rowg` = row + 4 g (so P1 of (s, kg) is rowg + s S1 + 256 kg and the row record row + 2 S1).
// (DT + GB_RP = the same format read from the repack: gemm_f16_plan.h)
struct RpHdr { u32x4 rec; uint32_t dd; };

template <> struct DeqI<NTK_DT_Q4_K + GB_RP> : GemmFmt<NTK_DT_Q4_K + GB_RP> {
    static constexpr int PPI = ITEM / 16, UB = 0, NCH = 0, NRING = 1;
    using Hdr = RpHdr;
    struct MinOp { uint32_t m0, m1; float ndmin64; };
    template <typename H> __device__ static MinOp min_operand(const H& hd, int g) {   // record bytes 8..15: m_0 .. m_7
        const uint32_t w = g == 0 ? hd.rec.z : (g == 1 ? hd.rec.w : 0u);
        return MinOp{cvt2_u8_f16<0>(w), cvt2_u8_f16<2>(w), -64.0f * h2f((uint16_t)(hd.dd >> 16))};
    }
    struct Raw { uint32_t lo, hi; float s0; };
    __device__ static Hdr header(const uint8_t* row, const uint8_t*) {
        const int i = threadIdx.x & 15;
        return Hdr{*reinterpret_cast<const u32x4*>(row + 2 * S1), *reinterpret_cast<const uint32_t*>(row + 2 * S1 + 256 - 12 * i)};
    }
    template <bool AL> __device__ static Raw load(const uint8_t*, const uint8_t* rowg, const Hdr& hd, int j, int) {
        const uint8_t* p = rowg + (j >> 2) * S1 + 512 * (j & 1);
        const uint32_t scw = j < 4 ? hd.rec.x : hd.rec.y;
        const float sc = (float)((scw >> (8 * (j & 3))) & 0xFFu);
        return Raw{lds32<true>(p), lds32<true>(p + 256), h2f((uint16_t)(hd.dd & 0xFFFFu)) * sc};
    }
    template <bool AL> __device__ static AOp convert(const Raw& r, int j, int) {
        const int sh = 4 * ((j >> 1) & 1);
        AOp o;
        o.a = cvt8_u8_f16((r.lo >> sh) & 0x0F0F0F0Fu, (r.hi >> sh) & 0x0F0F0F0Fu);
        o.s0 = o.s1 = r.s0;
        return o;
    }
};

template <> struct DeqI<NTK_DT_Q5_K + GB_RP> : GemmFmt<NTK_DT_Q5_K + GB_RP> {
    static constexpr int PPI = ITEM / 16, UB = 0, NCH = 0, NRING = 1;
    using Hdr = RpHdr;
    struct MinOp { uint32_t m0, m1; float ndmin64; };
    template <typename H> __device__ static MinOp min_operand(const H& hd, int g) {
        const uint32_t w = g == 0 ? hd.rec.z : (g == 1 ? hd.rec.w : 0u);
        return MinOp{cvt2_u8_f16<0>(w), cvt2_u8_f16<2>(w), -64.0f * h2f((uint16_t)(hd.dd >> 16))};
    }
    struct Raw { uint32_t lo, hi, b5lo, b5hi; float s0; };
    __device__ static Hdr header(const uint8_t* row, const uint8_t*) {
        const int i = threadIdx.x & 15;
        return Hdr{*reinterpret_cast<const u32x4*>(row + 2 * S1), *reinterpret_cast<const uint32_t*>(row + 2 * S1 + 256 - 12 * i)};
    }
    template <bool AL> __device__ static Raw load(const uint8_t* row, const uint8_t* rowg, const Hdr& hd, int j, int) {
        const int i = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3, h = (j >> 1) & 1;
        const uint8_t* p = rowg + (j >> 2) * S1 + 512 * (j & 1);
        // fifth bits: dword 16 kg + i of the step's 256-byte plane, bit 8 y + 4 h + v of column 4 v + y of the lane's chunk: this lane's four columns are v = g
        const uint8_t* f = row - 12 * i + (j >> 2) * S1 + 1024 + 128 * (j & 1);
        const uint32_t f0 = lds32<true>(f), f1 = lds32<true>(f + 64);
        const uint32_t scw = j < 4 ? hd.rec.x : hd.rec.y;
        const float sc = (float)((scw >> (8 * (j & 3))) & 0xFFu);
        return Raw{lds32<true>(p), lds32<true>(p + 256), ((f0 >> (4 * h + g)) & 0x01010101u) << 4, ((f1 >> (4 * h + g)) & 0x01010101u) << 4,
                   h2f((uint16_t)(hd.dd & 0xFFFFu)) * sc};
    }
    template <bool AL> __device__ static AOp convert(const Raw& r, int j, int) {
        const int sh = 4 * ((j >> 1) & 1);
        AOp o;
        o.a = cvt8_u8_f16(((r.lo >> sh) & 0x0F0F0F0Fu) | r.b5lo, ((r.hi >> sh) & 0x0F0F0F0Fu) | r.b5hi);
        o.s0 = o.s1 = r.s0;
        return o;
    }
};

template <> struct DeqI<NTK_DT_Q6_K + GB_RP> : GemmFmt<NTK_DT_Q6_K + GB_RP> {
    static constexpr int PPI = ITEM / 16, UB = 0, NCH = 0, NRING = 1;
    struct Hdr { u32x4 rec; float d; };   // sc[16] (int8), d
    struct MinOp {};
    __device__ static MinOp min_operand(const Hdr&, int) { return MinOp{}; }
    struct Raw { uint32_t lo, hi, b6lo, b6hi, sc; float d; };
    __device__ static Hdr header(const uint8_t* row, const uint8_t*) {
        const int i = threadIdx.x & 15;
        return Hdr{*reinterpret_cast<const u32x4*>(row + 2 * S1), h2f(*reinterpret_cast<const uint16_t*>(row + 2 * S1 + 256 - 14 * i))};
    }
    template <bool AL> __device__ static Raw load(const uint8_t* row, const uint8_t* rowg, const Hdr& hd, int j, int) {
        const int i = threadIdx.x & 15, g = (threadIdx.x >> 4) & 3, h = (j >> 1) & 1;
        const uint8_t* p = rowg + (j >> 2) * S1 + 512 * (j & 1);
        // bits 4..5: dwords 2 (16 kg + i) + h of the step's 512-byte plane, bits 8 y + 2 v (+1) of column 4 v + y: this lane's four columns are v = g
        const uint8_t* f = row - 8 * i + (j >> 2) * S1 + 1024 + 256 * (j & 1) + 4 * h;
        const uint32_t f0 = lds32<true>(f), f1 = lds32<true>(f + 128);
        const uint32_t scw = (j >> 1) == 0 ? hd.rec.x : (j >> 1) == 1 ? hd.rec.y : (j >> 1) == 2 ? hd.rec.z : hd.rec.w;   // sc[2 j], sc[2 j + 1]
        return Raw{lds32<true>(p), lds32<true>(p + 256), ((f0 >> (2 * g)) & 0x03030303u) << 4, ((f1 >> (2 * g)) & 0x03030303u) << 4,
                   (scw >> (16 * (j & 1))) & 0xFFFFu, hd.d};
    }
    template <bool AL> __device__ static AOp convert(const Raw& r, int j, int) {
        const int sh = 4 * ((j >> 1) & 1);
        const u32x4 qa = cvt8_u8_f16(((r.lo >> sh) & 0x0F0F0F0Fu) | r.b6lo, ((r.hi >> sh) & 0x0F0F0F0Fu) | r.b6hi);
        const f16x2 m32 = {(_Float16)-32.0f, (_Float16)-32.0f};
        auto sub32 = [&](uint32_t w) { return __builtin_bit_cast(uint32_t, (f16x2)(__builtin_bit_cast(f16x2, w) + m32)); };
        AOp o;   // q - 32: exact small integers
        o.a = u32x4{sub32(qa.x), sub32(qa.y), sub32(qa.z), sub32(qa.w)};
        o.s0 = r.d * (float)(int)(int8_t)(r.sc & 0xFF);
        o.s1 = r.d * (float)(int)(int8_t)(r.sc >> 8);
        return o;
    }
};

// Step timeline (tuning builds only: make trace): lane 0 of every wave of workgroup 0 records the shader clock before the step's
// wait, after its barrier and (level 2) once the step's LDS reads have returned; read back with ntk_debug_gemm_f16_trace(),
// printed by tools/gemm_f16_trace.py.  The stamps sit in LDS (a global store would join the vmcnt arithmetic).
#ifdef NTK_GEMM_TRACE   // (GBT_STEPS, GBT_EV, GB_TRACE_LDS: gemm_f16_plan.h)
__device__ unsigned long long g_gemm_f16_trace[4][GBT_STEPS][GBT_EV];
__device__ unsigned long long g_gemm_f16_clock[4];   // workgroup 0: shader clock and the constant 100 MHz clock at its first and last step
#define GB_STAMP(step, ev) do { if (gbt_on && (step) < GBT_STEPS) { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); \
        if (lane == 0) gbt[((size_t)wave * GBT_STEPS + (step)) * GBT_EV + (ev)] = t_; } } while (0)
#else
#define GB_STAMP(step, ev) do {} while (0)
#endif

// Ablation switches of tuning builds (wrong results, timing only): 1 = no MFMAs, 2 = no scale-FMAs (the MFMAs accumulate straight
// into the accumulators), 4 = no conversion of the raw weight dwords, 8 = no LDS reads of the activation planes, 16 = no activation
// DMA, 32 = no weight loads / staging.  0 in the product.
#ifndef NTK_GEMM_ABLATE
#define NTK_GEMM_ABLATE 0
#endif
constexpr int kGbAblate = NTK_GEMM_ABLATE;

// the scale-FMAs of a token-block pair one pair behind its MFMAs (two-chunk form of the formats without a minimum term): round 6, same box, alternated twice:
// 8B Q8_0 1024-token prompt 25 550 -> 26 400 tok/s (+3.3 %), gate | up 381 -> 363 us (profiles/r06_prompt_gemm_ab.txt).
constexpr bool GB_SWP = true;

struct GemmBSeg {
    const uint8_t* W;
    float* Y;               // [T][out]
    float* part;            // K split: [split][T][out] partial sums of this matrix
    int out, tile0;         // rows; first row tile of this matrix in the launch's tile numbering
    unsigned w_last;        // out * row_bytes - 16: the last 16-byte piece of the matrix (requests past the end re-read it)
    unsigned p2_off;        // repacked tensors (DT + GB_RP): byte offset of the row records behind the nibble planes; tiles of 16 rows
    int tiles16;
};
struct GemmBParams {
    GemmBSeg seg[GB_MAX_SEG];
    int nseg;
    const uint8_t* xb;      // operand planes [steps + 1][2][4][64] x 16 B
    const float* aux;       // [steps + 1][64]: sums of x s (K-quant minimum term)
    const float* inv;       // [T]: 1 / s of the launch's tokens
    const float* resid;     // optional [T][out] (single matrix only), may alias Y
    int T, in, steps;       // T = tokens of the launch (<= 16 chunks of 64)
    unsigned row_bytes;
    int nsplit, steps_per_split;   // blockIdx.y = K split; nsplit > 1: partial sums go to seg.part, summed by reduce_splits
    int chunks, row_wgs;    // 64-token chunks of this launch (blockIdx.x enumerates (row tile, chunk), see below); row tiles of all matrices
    int map8;               // blockIdx.x -> (row tile, chunk) in 8 x 8 blocks per XCD
    size_t chunk_bytes;     // between the planes (and sums) of consecutive chunks
};

// 16 B per lane, global -> LDS without passing through registers (gfx950 LDS-DMA, b128 form): lane l's 16 bytes land at
// M0 + imm + 16 l, read from gsrc + imm.  The compiler does not count these requests: the waits on them are explicit (vmcnt).
__device__ __forceinline__ void gb_dma16(uint32_t lds_dst, const uint8_t* gsrc) {
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}
__device__ __forceinline__ void gb_dma16x2(uint32_t lds_dst, const uint8_t* gsrc) {   // 2 KB per wave: +0, +1024 on both sides
    unsigned keep;
    asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\t"
                 "global_load_lds_dwordx4 %1, off offset:1024\n\ts_mov_b32 m0, %0"
                 : "=&s"(keep) : "v"(gsrc), "s"(lds_dst) : "memory");
}

// block = 256 threads = 4 waves; wave w of workgroup b owns weight rows (4 b + w) * 16 RT ... + 16 RT and all 64 tokens.
// MFMA roles: the activation planes are the A operand (M = 16 tokens), the weights the B operand (N = 16 weight rows), so the
// accumulator of lane (i, g) holds weight row i for tokens 4 g + e -- the row's scale is the one this lane decoded (no
// cross-lane traffic), and the step's sums of x / inverse scales come as float4s from LDS.
// One loop trip = GB_UPT units of SPU steps, straight-line (no exits inside: the s_waitcnt counts are exact).  Per step s:
//   wait until the DMA of step s has landed | barrier | at a unit's last step but one: the next unit's raw rows go from their ring
//   registers to the wave's LDS image and the ring slot is re-requested NRING units ahead | DMA step s + NS - 1 into the slot whose
//   planes were consumed a step ago | LDS reads: the step's sums, the raw weight dwords of step s + 2, the step's activation planes |
//   4 x (2 RT MFMAs, the token block's scale-FMAs), the conversion of step s + 1's weight operand in their shadow.
// CW = 2: the workgroup takes two consecutive 64-token chunks (128 tokens against every decoded weight: conversion, staging, barriers
// and weight traffic per MFMA halve); its planes are read a token-block pair at a time, one pair ahead of the MFMAs.
template <int DT, int RT, bool AL, bool PF, int CW>
__global__ __launch_bounds__(256, GB_WG_PER_CU) void gemm_quant_f16_kernel(const GemmBParams p) {
    using D = DeqI<DT>;
    constexpr int SPU = D::SPU, NCH = D::NCH, STRIDE = D::STRIDE;
    constexpr int ROWS = 16 * RT, PIECES = D::RP ? RT * D::PPI : ROWS * NCH, NLD = (PIECES + 63) / 64;   // 16-byte pieces of a unit; requests per lane
    constexpr int NRING = D::NRING;
    constexpr int NS = gb_slots<DT, RT, CW>();              // activation ring: slots
    constexpr int SLOT_BYTES = CW * GB_STEP_BYTES, NTB = 4 * CW;
    constexpr int XS_OFF = NS * SLOT_BYTES, STAGE_OFF = XS_OFF + gb_aux_lds<DT, CW>();
    static_assert(!D::HAS_MIN || (SPU == 8 && NS <= 8), "the minimum term's sums: units of 8 steps, two of them in LDS");
    static_assert(CW == 1 || (CW == 2 && !PF && !D::SPLIT16), "two chunks per workgroup: the pairwise plane pipeline, 32-column scales");
    static_assert(GB_UPT % NRING == 0 && NS >= 3 && NS - 2 <= GB_UPT * SPU, "a trip must cover whole turns of the weight ring");
    extern __shared__ __attribute__((aligned(16))) uint8_t gb_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    // blockIdx.x -> (row tile, token chunk).  Workgroups go to the 8 XCDs round-robin and every XCD takes its share in id order, 64 at a
    // time (2 per CU): XCD x owns the row tiles x, x + 8, ... and walks them in blocks of (8 row tiles) x (8 token chunks) -- the 64
    // workgroups resident on an XCD then share 8 weight streams and 8 activation streams through its L2 (per 32-column step 8 x 4.4 KB
    // + 8 x 8.3 KB leave the L2 towards the fabric; the round-2 order, all 16 chunks of 4 row tiles, 4 x 4.4 + 16 x 8.3 KB).
    const int bid = (int)blockIdx.x;
    const int xcd = bid & 7;
    int chunk, tile;
    if (p.map8) {
        int w = bid >> 3;
        const int tiles_x = (p.row_wgs + 7) >> 3;                       // row tiles of this XCD (the grid is padded to whole eights)
        const int ntg = (tiles_x + 7) >> 3, ncg = (p.chunks + 7) >> 3;
        const int tg = min(w / (8 * p.chunks), ntg - 1);
        w -= tg * 8 * p.chunks;
        const int tsz = min(8, tiles_x - 8 * tg);
        const int cg = min(w / (tsz * 8), ncg - 1);
        w -= cg * tsz * 8;
        const int csz = min(8, p.chunks - 8 * cg);
        chunk = 8 * cg + w % csz;
        tile = (8 * tg + w / csz) * 8 + xcd;
    } else {   // (NTK_GEMM_MAP=0: the chunks of a row tile 8 ids apart, tile after tile)
        const int within = bid >> 3;
        chunk = within % p.chunks;
        tile = (within / p.chunks) * 8 + xcd;
    }
    if (tile >= p.row_wgs) return;   // row tiles are padded to a multiple of 8
#ifdef NTK_GEMM_TRACE
    unsigned long long* gbt = reinterpret_cast<unsigned long long*>(gb_lds + STAGE_OFF + 4 * 16 * RT * DeqI<DT>::STRIDE);
    const bool gbt_on = bid == 0 && blockIdx.y == 0;
    if (gbt_on) for (int q = tid; q < 4 * GBT_STEPS * GBT_EV; q += 256) gbt[q] = 0;
    if (gbt_on && tid == 0) { g_gemm_f16_clock[0] = __builtin_amdgcn_s_memtime(); g_gemm_f16_clock[1] = __builtin_amdgcn_s_memrealtime(); }
#endif
    // which matrix of the launch this row tile belongs to (workgroup-uniform)
    int sidx = 0;
    if (p.nseg > 1 && tile >= p.seg[1].tile0) sidx = 1;
    if (p.nseg > 2 && tile >= p.seg[2].tile0) sidx = 2;
    const uint8_t* const segW = p.seg[sidx].W;
    float* const segY = p.seg[sidx].Y;
    float* const segPart = p.seg[sidx].part;
    const int seg_out = p.seg[sidx].out;
    const unsigned seg_w_last = p.seg[sidx].w_last;
    chunk *= CW;   // the workgroup's first 64-token chunk (p.chunks counts workgroup-sized groups)
    const int Tc = min(CW * GB_TOK, p.T - chunk * GB_TOK);
    const int row0 = ((tile - p.seg[sidx].tile0) * 4 + wave) * ROWS;
    f32x4 acc[RT][NTB];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int tb = 0; tb < NTB; ++tb) acc[rt][tb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    // this workgroup's K range (split-K: blockIdx.y), in steps of 32 columns; whole trips of GB_UPT * SPU steps
    const int step_lo = (int)blockIdx.y * p.steps_per_split, step_hi = min(p.steps, step_lo + p.steps_per_split);
    const int nsteps = step_hi - step_lo;
    const int unit_lo = step_lo / SPU, nunits = (nsteps + SPU - 1) / SPU;

    // weight pieces of this lane: piece q = 64 n + lane of the wave's unit -> row q / NCH, 16-byte piece q % NCH of the 16-byte
    // aligned window that covers the row's unit (rows need not be 16-byte aligned: every row has its own window start and shift)
    uint8_t* stage = gb_lds + STAGE_OFF + (size_t)wave * (ROWS * STRIDE);
    uint32_t w_row[NLD], s_pk[NLD];   // s_pk: offset of the piece in the wave's image | 16 c << 16 (unpacked once per unit: registers are the scarcer resource)
    if constexpr (D::RP) {   // piece q of the wave's RT items: item rt = q / PPI, 16-byte piece q % PPI of [P1 | P2]; s_pk = image offset | bytes per unit << 16
        const unsigned nsb = (unsigned)(p.in / 256);
#pragma unroll
        for (int n = 0; n < NLD; ++n) {
            const int q = min(64 * n + lane, PIECES - 1), rt = q / D::PPI, idx = q - rt * D::PPI;
            const unsigned tile = (unsigned)min(row0 / 16 + rt, p.seg[sidx].tiles16 - 1);
            const bool rec = idx >= 2 * D::S1 / 16;
            w_row[n] = rec ? p.seg[sidx].p2_off + tile * nsb * (unsigned)D::S2 + 16u * (unsigned)(idx - 2 * D::S1 / 16) : tile * nsb * (unsigned)(2 * D::S1) + 16u * (unsigned)idx;
            s_pk[n] = (uint32_t)(rt * D::ITEM + 16 * idx) | ((uint32_t)(rec ? D::S2 : 2 * D::S1) << 16);
        }
    } else {
#pragma unroll
    for (int n = 0; n < NLD; ++n) {
        const int q = min(64 * n + lane, PIECES - 1), r = q / NCH, c = q - r * NCH;
        w_row[n] = (uint32_t)min(row0 + r, seg_out - 1) * p.row_bytes;
        s_pk[n] = (uint32_t)(r * STRIDE + 16 * c) | ((uint32_t)(16 * c) << 16);
    }
    }
    // The ring's loads and the stores that consume them are inline asm: a load the compiler tracks makes it wait, at the consumer, for
    // "all but the tracked loads younger than it" -- it does not see the LDS-DMA requests in between, so that wait drained the whole
    // activation ring at every unit boundary (round 3, the ISA of the first deep-ring build).  Here every wait is explicit and exact.
    // (The ring registers appear in no compiler-generated instruction: tools/check_gemm_isa.py checks the build for that.)
    u32x4 ring[NRING][NLD];
    auto load_unit = [&](int k, int urel) {   // unit `urel` of this split (past the end: the last one again, multiplied by zeros)
        if (kGbAblate & 32) { if (urel >= 2) return; }
        const uint32_t uoff = (uint32_t)(unit_lo + min(urel, nunits - 1)) * D::UB;
#pragma unroll
        for (int n = 0; n < NLD; ++n) {
            uint32_t off;
            if constexpr (D::RP) off = w_row[n] + (uint32_t)(unit_lo + min(urel, nunits - 1)) * (s_pk[n] >> 16);   // (tiles are padded: every piece exists)
            else off = min(((w_row[n] + uoff) & ~15u) + (s_pk[n] >> 16), seg_w_last);
            asm volatile("global_load_dwordx4 %0, %1, %2" : "=v"(ring[k][n]) : "v"(off), "s"(segW) : "memory");
        }
    };
    // (the caller waits first: s_waitcnt vmcnt(requests issued after the unit's loads))
    auto stage_unit = [&](int k) {
        if (kGbAblate & 32) return;
#pragma unroll
        for (int n = 0; n < NLD; ++n)
            asm volatile("ds_write_b128 %0, %1" ::"v"((uint32_t)(uintptr_t)(stage + (s_pk[n] & 0xFFFFu))), "v"(ring[k][n]) : "memory");
    };

    const uint32_t lds0 = (uint32_t)(uintptr_t)gb_lds;   // generic -> LDS address: the low 32 bits
    const uint8_t* xb_thread = p.xb + (size_t)chunk * p.chunk_bytes + (size_t)wave * 2048 + (size_t)lane * 16;   // wave w copies bytes [2048 w, 2048 w + 2048) of a step record
    const uint8_t* aux_thread = reinterpret_cast<const uint8_t*>(p.aux) + (size_t)chunk * p.chunk_bytes + (size_t)wave * 64 + (size_t)(lane & 3) * 16;   // and 64 of its 256 aux bytes
    constexpr int ND = CW * (D::HAS_MIN ? 3 : 2);        // DMA requests per step and wave
    // dpos = the destination step's position in its pair of units (0..15, compile time at every call): the step's eighth of its unit's record
    // of sums goes to buffer dpos / 8
    auto dma_step = [&](int rel, int slot, int dpos) {   // step record `rel` (past the end: the record of zeros) into ring slot `slot` (uniform)
        if ((kGbAblate & 16) && rel >= NS - 1) return;
        const int s = rel < nsteps ? step_lo + rel : p.steps;
#pragma unroll
        for (int c = 0; c < CW; ++c) {   // (a second chunk past the end of the launch reads planes nobody wrote: its tokens are never stored)
            gb_dma16x2(__builtin_amdgcn_readfirstlane(lds0 + (uint32_t)slot * SLOT_BYTES + (uint32_t)c * GB_STEP_BYTES + (uint32_t)wave * 2048u),
                       xb_thread + (size_t)c * p.chunk_bytes + (size_t)s * GB_STEP_BYTES);
            if (D::HAS_MIN && lane < 4)   // 64 of the eighth's 256 bytes per wave (one request: the vmcnt arithmetic counts it for every lane)
                gb_dma16(__builtin_amdgcn_readfirstlane(lds0 + XS_OFF + (uint32_t)c * (2 * GB_MIN_UNIT_BYTES) + (uint32_t)(dpos >> 3) * GB_MIN_UNIT_BYTES +
                                                        (uint32_t)(dpos & 7) * GB_AUX_BYTES + (uint32_t)wave * 64u),
                         aux_thread + (size_t)c * p.chunk_bytes + (size_t)s * GB_AUX_BYTES);
        }
    };
    const uint8_t* img[RT];      // this lane's row images (row rt*16 + i of the wave's tile)
    uint32_t my_row[RT];         // and the rows' byte offsets in W: the unit's bytes start `(my_row + unit offset) & 15` into the image
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        img[rt] = D::RP ? stage + rt * D::ITEM + 16 * i : stage + (rt * 16 + i) * STRIDE;
        my_row[rt] = (uint32_t)min(row0 + rt * 16 + i, seg_out - 1) * p.row_bytes;
    }
    typename D::Hdr hdr[RT];
    typename D::MinOp mcur[RT], mnext[RT];   // K-quant minima of the unit whose steps run / of the unit entered two steps before its first
    const uint8_t* cur[RT];      // img + the staged unit's shift (AL: rounded down to a dword boundary)
    auto enter_unit = [&](int unit) {   // the image now holds `unit`
        const uint32_t uoff = (uint32_t)(unit_lo + min(unit, nunits - 1)) * D::UB;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const uint8_t* first = D::RP ? img[rt] : img[rt] + ((my_row[rt] + uoff) & 15u);   // (the repack's items lie in the image as they are)
            hdr[rt] = D::header(first, first + 4 * g);
            mnext[rt] = D::min_operand(hdr[rt], g);
            cur[rt] = D::RP ? first : (AL ? img[rt] + ((my_row[rt] + uoff) & 12u) : first);
        }
    };
    auto read_planes = [&](u32x4 (&b)[GB_PLANES][4], int slot) {   // token block by token block: the order the MFMAs take them in
        const u32x4* bs = reinterpret_cast<const u32x4*>(gb_lds + (size_t)slot * SLOT_BYTES) + lane;
#pragma unroll
        for (int tb = 0; tb < 4; ++tb)
#pragma unroll
            for (int pl = 0; pl < GB_PLANES; ++pl) b[pl][tb] = bs[(pl * 4 + tb) * 64];
    };
    // Prologue: the weight ring; unit 0 staged and its ring slot re-requested; the DMAs of steps 0 .. NS - 2; everything landed (one
    // memory round trip per workgroup: from here on the waits count the requests of the loop's own steps, which come in a fixed order);
    // step 0 loaded and converted, step 1 loaded.
#pragma unroll
    for (int k = 0; k < NRING; ++k) load_unit(k, k);
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NRING - 1) * NLD) : "memory");
    stage_unit(0);
    load_unit(0, NRING);
#pragma unroll
    for (int q = 0; q < NS - 1; ++q) dma_step(q, q, q);
    static_assert(SPU >= 4, "units of >= 4 steps: steps 0 and 1 belong to unit 0");
    enter_unit(0);
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) mcur[rt] = mnext[rt];
    AOp a[RT];
    typename D::Raw rawn[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        a[rt] = D::template convert<AL>(D::template load<AL>(cur[rt], cur[rt] + 4 * g, hdr[rt], 0, 0), 0, 0);
        rawn[rt] = D::template load<AL>(cur[rt], cur[rt] + 4 * g, hdr[rt], 1, 0);
    }
    asm volatile("s_waitcnt vmcnt(0)\n\ts_barrier" ::: "memory");
    int slot = 0;   // ring slot of the current step (uniform)
    u32x4 b[GB_PLANES][4];
    if constexpr (PF) read_planes(b, 0);   // PF: a step's planes are read one step ahead of its MFMAs, into a second register set
    // CW = 2: token blocks 2 q, 2 q + 1 of a slot -> one of two register sets of 4 operands ([plane][block of the pair])
    auto read_pair = [&](u32x4 (&bq)[GB_PLANES][2], int slot, int q) {
        const u32x4* bs = reinterpret_cast<const u32x4*>(gb_lds + (size_t)slot * SLOT_BYTES + (size_t)(q >> 1) * GB_STEP_BYTES) + lane;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
            for (int pl = 0; pl < GB_PLANES; ++pl) bq[pl][t2] = bs[(pl * 4 + (q & 1) * 2 + t2) * 64];
    };

    f32x4 carry[RT][2];   // (GB_SWP, CW = 2) the step's last pair of block sums, scaled at the head of the next step
    float s_carry[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        s_carry[rt] = 0.0f;
#pragma unroll
        for (int t2 = 0; t2 < 2; ++t2) carry[rt][t2] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    }
    for (int trip = 0; trip * (GB_UPT * SPU) < nsteps; ++trip) {
#pragma unroll
        for (int k = 0; k < GB_UPT; ++k) {
#pragma unroll
            for (int j = 0; j < SPU; ++j) {
                const int rel = (trip * GB_UPT + k) * SPU + j;        // step relative to the split's start
                GB_STAMP(rel, 0);
                // The DMA of the step whose planes are read now (this step; PF: the next one) went out NS - 1 (NS - 2) steps ago.  Younger
                // requests: the DMAs of the steps since and the next unit's weight requests of every step SPU - 2 among them (they go out
                // ahead of that step's DMA).  (In the first steps of the launch the count is too high for what is really in flight -- but
                // what they wait for landed in the prologue.)
                {
                    constexpr int T = GB_UPT * SPU, BACK = PF ? NS - 3 : NS - 2;
                    int nload = 0;
#pragma unroll
                    for (int d = 1; d <= BACK; ++d) nload += (((k * SPU + j - d) % T + T) % T) % SPU == SPU - 2 ? 1 : 0;
                    // (nload is a compile-time constant after unrolling: one asm statement per value)
                    if (nload == 0) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(BACK * ND) : "memory");
                    else if (nload == 1) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(BACK * ND + NLD) : "memory");
                    else if (nload == 2) asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(BACK * ND + 2 * NLD) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)\n\ts_barrier" ::"n"(BACK * ND + 3 * NLD) : "memory");
                    static_assert((BACK + SPU - 1) / SPU <= 3, "at most three weight request groups in flight behind a DMA");
                }
                GB_STAMP(rel, 1);
                if (j == SPU - 2) {   // the raw dwords of this unit's last step were read a step ago: the image is free for the next unit
                    // younger than the loads of the unit staged now: the DMAs of the NRING * SPU steps since, the loads of the other ring slots
                    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NRING * SPU * ND + (NRING - 1) * NLD) : "memory");
                    stage_unit((k + 1) % NRING);
                    load_unit((k + 1) % NRING, trip * GB_UPT + k + 1 + NRING);
                    enter_unit(trip * GB_UPT + k + 1);
                }
                // into the slot of step rel - 1: its planes were read a step ago and consumed before this barrier
                dma_step(rel + NS - 1, slot == 0 ? NS - 1 : slot - 1, (k * SPU + j + NS - 1) % (GB_UPT * SPU));
                // ---- one scheduling region from here to the end of the step ----
                // LDS reads, in the order their consumers come: the raw weight dwords of the step after next, the activation planes
                typename D::Raw raw2[RT];
                {
                    const int j2 = (j + 2) % SPU, k2 = (j + 2 >= SPU) ? (k + 1) % GB_UPT : k;   // (cur / hdr already belong to the next unit from step SPU - 2 on)
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) raw2[rt] = D::template load<AL>(cur[rt], cur[rt] + 4 * g, hdr[rt], j2, k2);
                }
                u32x4 bn[GB_PLANES][4];
                u32x4 bq[2][GB_PLANES][2];
                if constexpr (CW == 2) read_pair(bq[0], slot, 0);
                else if constexpr (PF) read_planes(bn, slot == NS - 1 ? 0 : slot + 1);
                else if (!(kGbAblate & 8) || rel == 0) read_planes(b, slot);
#if defined(NTK_GEMM_TRACE) && NTK_GEMM_TRACE > 1
                GB_STAMP(rel, 2);
#endif
                // the next step's operand out of the dwords read a step ago: VALU work with no LDS read of this step behind it
                AOp an[RT];
                {
                    const int j1 = (j + 1) % SPU, k1 = (j + 1 >= SPU) ? (k + 1) % GB_UPT : k;
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt) {
                        if (kGbAblate & 4) {   // the raw dwords as they are
                            uint32_t w[sizeof(typename D::Raw) / 4];
                            __builtin_memcpy(w, &rawn[rt], sizeof(w));
                            an[rt].a = u32x4{w[0], w[1], w[2 % (sizeof(w) / 4)], w[3 % (sizeof(w) / 4)]};
                            an[rt].s0 = an[rt].s1 = __uint_as_float(w[sizeof(w) / 4 - 1]);
                        } else an[rt] = D::template convert<AL>(rawn[rt], j1, k1);
                    }
                }
                // MFMAs token block by token block; a block's scale-FMAs follow its chains and hide under the next block's MFMAs
                if constexpr (D::SPLIT16) {   // two 16-column groups with their own scale: K = 16 MFMAs on the operand halves
#pragma unroll
                    for (int tb = 0; tb < 4; ++tb) {
                        f32x4 cl[RT], ch[RT];
#pragma unroll
                        for (int pl = 0; pl < GB_PLANES; ++pl) {
                            const f16x4 xl = __builtin_bit_cast(f16x4, (uint64_t)b[pl][tb].x | ((uint64_t)b[pl][tb].y << 32));
                            const f16x4 xh = __builtin_bit_cast(f16x4, (uint64_t)b[pl][tb].z | ((uint64_t)b[pl][tb].w << 32));
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt) {
                                const f16x4 wl = __builtin_bit_cast(f16x4, (uint64_t)a[rt].a.x | ((uint64_t)a[rt].a.y << 32));
                                const f16x4 wh = __builtin_bit_cast(f16x4, (uint64_t)a[rt].a.z | ((uint64_t)a[rt].a.w << 32));
                                const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                                cl[rt] = __builtin_amdgcn_mfma_f32_16x16x16f16(xl, wl, pl ? cl[rt] : z, 0, 0, 0);
                                ch[rt] = __builtin_amdgcn_mfma_f32_16x16x16f16(xh, wh, pl ? ch[rt] : z, 0, 0, 0);
                            }
                        }
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                            for (int e = 0; e < 4; ++e)
                                acc[rt][tb][e] = fmaf(a[rt].s1, ch[rt][e], fmaf(a[rt].s0, cl[rt][e], acc[rt][tb][e]));
                    }
                } else if constexpr (CW == 2 && GB_SWP && (!D::HAS_MIN || D::RP)) {   // (the raw K-quant decoders have no registers left for it; the repack decoders do)
                    // four pairs of token blocks, the scale-FMAs of a pair one pair BEHIND its MFMAs (GB_SWP): an FMA issued right behind the
                    // chain it reads waits out the matrix pipe's latency (the build without this: an s_nop 7 in front of every group of four);
                    // here the FMAs that sit between a pair's MFMAs read the previous pair's finished sums.  The step's last pair is scaled at the
                    // head of the NEXT step (carry[] / s_carry[]; the first step scales zeros by zero), the very last one behind the loop.
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (q < 3) read_pair(bq[(q + 1) & 1], slot, q + 1);
                        f32x4 cc[RT][2];
#pragma unroll
                        for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                            for (int pl = 0; pl < GB_PLANES; ++pl)
#pragma unroll
                                for (int rt = 0; rt < RT; ++rt) {
                                    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                                    cc[rt][t2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, bq[q & 1][pl][t2]), __builtin_bit_cast(f16x8, a[rt].a),
                                                                                        pl ? cc[rt][t2] : z, 0, 0, 0);
                                }
                        // the pair before this one (q = 0: the previous step's last pair, under its scales)
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) {
                            const float sc = q == 0 ? s_carry[rt] : a[rt].s0;
#pragma unroll
                            for (int t2 = 0; t2 < 2; ++t2) {
                                const int tb = q == 0 ? 6 + t2 : 2 * (q - 1) + t2;
#pragma unroll
                                for (int e = 0; e < 4; ++e) acc[rt][tb][e] = fmaf(sc, carry[rt][t2][e], acc[rt][tb][e]);
                            }
                        }
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
                            for (int t2 = 0; t2 < 2; ++t2) carry[rt][t2] = cc[rt][t2];
                            if (q == 3) s_carry[rt] = a[rt].s0;
                        }
                        __builtin_amdgcn_sched_group_barrier(0x100, 64, 0);
#pragma unroll
                        for (int n = 0; n < 2 * GB_PLANES * RT; ++n) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                    if constexpr (D::HAS_MIN) {
                        // a unit's last step: its last pair is scaled HERE, in front of the minimum term below -- the order of additions into every accumulator
                        // stays the one of the form without the carry (and of the raw-GGUF decoders: identical bits); the next step's head then adds 0 * carry
                        if (j == SPU - 1) {
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
                                for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                                    for (int e = 0; e < 4; ++e) acc[rt][6 + t2][e] = fmaf(s_carry[rt], carry[rt][t2][e], acc[rt][6 + t2][e]);
                                s_carry[rt] = 0.0f;
                            }
                        }
                    }
                } else if constexpr (CW == 2) {
                    // four pairs of token blocks: the next pair's planes are requested before this pair's MFMAs go out
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        if (q < 3) read_pair(bq[(q + 1) & 1], slot, q + 1);
#pragma unroll
                        for (int t2 = 0; t2 < 2; ++t2) {
                            const int tb = 2 * q + t2;
                            f32x4 cc[RT];
#pragma unroll
                            for (int pl = 0; pl < GB_PLANES; ++pl)
#pragma unroll
                                for (int rt = 0; rt < RT; ++rt) {
                                    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                                    cc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, bq[q & 1][pl][t2]), __builtin_bit_cast(f16x8, a[rt].a),
                                                                                    pl ? cc[rt] : z, 0, 0, 0);
                                }
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                                for (int e = 0; e < 4; ++e) {
                                    float v = fmaf(a[rt].s0, cc[rt][e], acc[rt][tb][e]);
                                    acc[rt][tb][e] = v;
                                }
                        }
                        // the pair's region: its LDS reads (and, q = 0, the step's other reads) first, then MFMAs with VALU work in their shadow
                        __builtin_amdgcn_sched_group_barrier(0x100, 64, 0);
#pragma unroll
                        for (int n = 0; n < 2 * GB_PLANES * RT; ++n) {
                            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                            __builtin_amdgcn_sched_group_barrier(0x002, 4, 0);
                        }
                        __builtin_amdgcn_sched_barrier(0);
                    }
                } else {
#pragma unroll
                    for (int tb = 0; tb < 4; ++tb) {
                        f32x4 cc[RT];
#pragma unroll
                        for (int pl = 0; pl < GB_PLANES; ++pl)
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt) {
                                const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                                if (kGbAblate & 1) cc[rt] = __builtin_bit_cast(f32x4, b[pl][tb]);
                                else if (kGbAblate & 2) acc[rt][tb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, b[pl][tb]), __builtin_bit_cast(f16x8, a[rt].a), acc[rt][tb], 0, 0, 0);
                                else cc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, b[pl][tb]), __builtin_bit_cast(f16x8, a[rt].a),
                                                                                pl ? cc[rt] : z, 0, 0, 0);
                            }
                        if (!(kGbAblate & 2))
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                            for (int e = 0; e < 4; ++e) {
                                float v = fmaf(a[rt].s0, cc[rt][e], acc[rt][tb][e]);
                                acc[rt][tb][e] = v;
                            }
                    }
                }
                // issue order of the region: every LDS read first, then the MFMAs with VALU work in their shadow
                if constexpr (CW == 1) {
                    constexpr int NMF = (D::SPLIT16 ? 8 : 4) * GB_PLANES * RT;
                    __builtin_amdgcn_sched_group_barrier(0x100, 64, 0);
#pragma unroll
                    for (int n = 0; n < NMF; ++n) {
                        __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                        __builtin_amdgcn_sched_group_barrier(0x002, D::SPLIT16 ? 2 : 4, 0);
                    }
                }
                // K-quant minimum of the unit that ends here (gemm.cu:232-244: - dmin m_j sum_k x_k per sub-block j): sum_j m_j S_j over the
                // unit's 8 sub-blocks is one K = 8 product per (row, token) -- two MFMAs per tile (the two FP16 pieces of S / 64: lane
                // (token, g < 2) holds steps 4 g .. 4 g + 3; the weight-side operand holds m_j there and zeros elsewhere, so whatever
                // finite values sit in the rest of the token-side operand do not count), then one FMA per element with -64 dmin.
                // Per step that was 2 packed FMAs per tile and a 16-byte LDS read per token block.
                if constexpr (D::HAS_MIN) {
                    if (j == SPU - 1) {
#pragma unroll
                        for (int tb = 0; tb < NTB; ++tb) {
                            const uint8_t* rec = gb_lds + XS_OFF + (tb >> 2) * (2 * GB_MIN_UNIT_BYTES) + k * GB_MIN_UNIT_BYTES + (((tb & 3) * 2 + (g & 1)) * 16 + i) * 8;
                            f32x4 rr[RT];
#pragma unroll
                            for (int pl = 0; pl < GB_PLANES; ++pl) {
                                const uint64_t sv = *reinterpret_cast<const uint64_t*>(rec + pl * (GB_MIN_UNIT_BYTES / 2));
                                const u32x4 sa = {(uint32_t)sv, (uint32_t)(sv >> 32), (uint32_t)sv, (uint32_t)(sv >> 32)};
#pragma unroll
                                for (int rt = 0; rt < RT; ++rt) {
                                    const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                                    const u32x4 mb = {mcur[rt].m0, mcur[rt].m1, 0u, 0u};
                                    rr[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, sa), __builtin_bit_cast(f16x8, mb), pl ? rr[rt] : z, 0, 0, 0);
                                }
                            }
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                                for (int e = 0; e < 4; ++e) acc[rt][tb][e] = fmaf(mcur[rt].ndmin64, rr[rt][e], acc[rt][tb][e]);
                        }
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) mcur[rt] = mnext[rt];
                    }
                }
                // the accumulators and the next operands are complete HERE: without this anchor the instruction selector parks every
                // step's scale-FMAs at the end of the trip (they have no memory dependence) and the products of 16 steps sit in
                // registers until then
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) {
#pragma unroll
                    for (int tb = 0; tb < NTB; ++tb) asm volatile("" : "+v"(acc[rt][tb]));
                    a[rt] = an[rt];
                    asm volatile("" : "+v"(a[rt].a), "+v"(a[rt].s0), "+v"(a[rt].s1));
                    rawn[rt] = raw2[rt];
                }
                if constexpr (PF) {
#pragma unroll
                    for (int pl = 0; pl < GB_PLANES; ++pl)
#pragma unroll
                        for (int tb = 0; tb < 4; ++tb) b[pl][tb] = bn[pl][tb];
                }
                slot = slot == NS - 1 ? 0 : slot + 1;
                __builtin_amdgcn_sched_barrier(0);   // no motion of memory requests across steps (the waits count them in order)
            }
        }
    }
    if constexpr (CW == 2 && GB_SWP && (!D::HAS_MIN || D::RP) && !D::SPLIT16) {   // the last step's last pair
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int t2 = 0; t2 < 2; ++t2)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[rt][6 + t2][e] = fmaf(s_carry[rt], carry[rt][t2][e], acc[rt][6 + t2][e]);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // no DMA may still be in flight towards LDS when the workgroup retires
#ifdef NTK_GEMM_TRACE
    if (gbt_on) {
        if (tid == 0) { g_gemm_f16_clock[2] = __builtin_amdgcn_s_memtime(); g_gemm_f16_clock[3] = __builtin_amdgcn_s_memrealtime(); }
        __syncthreads();
        for (int q = tid; q < 4 * GBT_STEPS * GBT_EV; q += 256) (&g_gemm_f16_trace[0][0][0])[q] = gbt[q];
    }
#endif
    // ---- epilogue: accumulator element e of lane (i = weight row of the tile, g) is token tb*16 + 4g + e of the chunk; 1 / s ------
    const size_t tok0 = (size_t)chunk * GB_TOK;
    f32x4 inv_t[NTB];
#pragma unroll
    for (int tb = 0; tb < NTB; ++tb) inv_t[tb] = *reinterpret_cast<const f32x4*>(p.inv + tok0 + tb * 16 + 4 * g);   // (the array is padded to whole chunks)
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        const int r = row0 + rt * 16 + i;
        if (r >= seg_out) continue;
        if (p.nsplit > 1) {   // K split: this workgroup's partial sums, combined (fixed order) by reduce_splits_kernel
#pragma unroll
            for (int tb = 0; tb < NTB; ++tb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int t = tb * 16 + 4 * g + e;
                    if (t < Tc) segPart[((size_t)blockIdx.y * p.T + tok0 + t) * seg_out + r] = acc[rt][tb][e] * inv_t[tb][e];
                }
            continue;
        }
        float rs[NTB][4];
#pragma unroll
        for (int tb = 0; tb < NTB; ++tb)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int t = tb * 16 + 4 * g + e;
                rs[tb][e] = (p.resid && t < Tc) ? p.resid[(tok0 + t) * seg_out + r] : 0.0f;
            }
#pragma unroll
        for (int tb = 0; tb < NTB; ++tb)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int t = tb * 16 + 4 * g + e;
                if (t < Tc) segY[(tok0 + t) * seg_out + r] = acc[rt][tb][e] * inv_t[tb][e] + rs[tb][e];
            }
    }
}

// ---- short prompts (<= 32 tokens): the same arithmetic as a WEIGHT-STREAMING kernel (round 6) ------------------------------------------------------------
// The kernel above is built for the matrix pipe: per 32-column step a workgroup barrier, an LDS-DMA record of activation planes, a latency of ~1 us that 128
// tokens of MFMAs hide.  With 16 or 32 tokens there is nothing to hide it behind -- the step costs the same and the launch streams its weights at 1-2 TB/s
// (8B Q8_0: a 16-token prompt 7.2 ms, a 64-token one 6.3 ms, a decode token 1.8 ms).  This form is the decode GEMV's structure around the GEMM's operands:
//   * a workgroup owns 16 RT rows; its NW waves split K in whole units, every wave streams ITS slice of the rows (the loader and the per-wave LDS image
//     of the kernel above, the decoders DeqI<DT> -- raw GGUF or the decode repack -- unchanged) and keeps its own accumulators: no barrier in the loop;
//   * the activation planes of a step (1 KiB per plane and 16-token block: one 16-byte load per lane) come straight from L2 into the MFMA operand
//     registers, one step ahead -- every workgroup reads the same 4 in bytes per token, they never leave the XCDs' L2s;
//   * the waves' partial sums meet in LDS once, in wave order (deterministic), times 1 / s, + residual.
// Same products and scales as the kernel above; the summation order differs (K is cut per wave): parity at the GEMV tolerance, not bit equality.
struct GemmSParams {
    GemmBSeg seg[GB_MAX_SEG];
    int nseg;
    const uint8_t* xb;      // operand planes of the (single) chunk
    const uint8_t* aux;     // its step sums (K-quant minimum term)
    const float* inv;       // [T]: 1 / s
    const float* resid;
    int T, in, steps;
    unsigned row_bytes;
};

template <int DT, int RT, int NTB, bool AL>
__global__ __launch_bounds__(512) void gemm_quant_f16_small_kernel(const GemmSParams p) {
    using D = DeqI<DT>;
    constexpr int SPU = D::SPU, NCH = D::NCH, STRIDE = D::STRIDE;
    constexpr int ROWS = 16 * RT, PIECES = D::RP ? RT * D::PPI : ROWS * NCH, NLD = (PIECES + 63) / 64;
    extern __shared__ __attribute__((aligned(16))) uint8_t gs_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), NW = (int)(blockDim.x >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int tile = (int)blockIdx.x;
    int sidx = 0;
    if (p.nseg > 1 && tile >= p.seg[1].tile0) sidx = 1;
    if (p.nseg > 2 && tile >= p.seg[2].tile0) sidx = 2;
    const uint8_t* const segW = p.seg[sidx].W;
    const int seg_out = p.seg[sidx].out;
    const unsigned seg_w_last = p.seg[sidx].w_last;
    const int row0 = (tile - p.seg[sidx].tile0) * ROWS;
    // this wave's units
    const int U = p.steps / SPU, ub = U / NW, ur = U - ub * NW;
    const int u_lo = wave * ub + min(wave, ur), u_hi = u_lo + ub + (wave < ur ? 1 : 0);
    uint8_t* stage = gs_lds + (size_t)wave * (ROWS * STRIDE);
    uint32_t w_row[NLD], s_pk[NLD];
    if constexpr (D::RP) {
        const unsigned nsb = (unsigned)(p.in / 256);
#pragma unroll
        for (int n = 0; n < NLD; ++n) {
            const int q = min(64 * n + lane, PIECES - 1), rt = q / D::PPI, idx = q - rt * D::PPI;
            const unsigned t16 = (unsigned)min(row0 / 16 + rt, p.seg[sidx].tiles16 - 1);
            const bool rec = idx >= 2 * D::S1 / 16;
            w_row[n] = rec ? p.seg[sidx].p2_off + t16 * nsb * (unsigned)D::S2 + 16u * (unsigned)(idx - 2 * D::S1 / 16) : t16 * nsb * (unsigned)(2 * D::S1) + 16u * (unsigned)idx;
            s_pk[n] = (uint32_t)(rt * D::ITEM + 16 * idx) | ((uint32_t)(rec ? D::S2 : 2 * D::S1) << 16);
        }
    } else {
#pragma unroll
        for (int n = 0; n < NLD; ++n) {
            const int q = min(64 * n + lane, PIECES - 1), r = q / NCH, c = q - r * NCH;
            w_row[n] = (uint32_t)min(row0 + r, seg_out - 1) * p.row_bytes;
            s_pk[n] = (uint32_t)(r * STRIDE + 16 * c) | ((uint32_t)(16 * c) << 16);
        }
    }
    auto load_unit = [&](u32x4 (&w)[NLD], int unit) {
#pragma unroll
        for (int n = 0; n < NLD; ++n) {
            uint32_t off;
            if constexpr (D::RP) off = w_row[n] + (uint32_t)unit * (s_pk[n] >> 16);
            else off = min(((w_row[n] + (uint32_t)unit * D::UB) & ~15u) + (s_pk[n] >> 16), seg_w_last);
            w[n] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(segW + off));
        }
    };
    const uint8_t* img[RT];
    uint32_t my_row[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        img[rt] = D::RP ? stage + rt * D::ITEM + 16 * i : stage + (rt * 16 + i) * STRIDE;
        my_row[rt] = (uint32_t)min(row0 + rt * 16 + i, seg_out - 1) * p.row_bytes;
    }
    const u32x4* xb = reinterpret_cast<const u32x4*>(p.xb) + lane;   // + (step * 8 + plane * 4 + token block) * 64
    f32x4 acc[RT][NTB];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int tb = 0; tb < NTB; ++tb) acc[rt][tb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    auto load_planes = [&](u32x4 (&b)[GB_PLANES][NTB], int step) {
#pragma unroll
        for (int pl = 0; pl < GB_PLANES; ++pl)
#pragma unroll
            for (int tb = 0; tb < NTB; ++tb) b[pl][tb] = xb[(size_t)((step * GB_PLANES + pl) * 4 + tb) * 64];
    };
    if (u_lo < u_hi) {
        u32x4 wreg[NLD];
        load_unit(wreg, u_lo);
        u32x4 bn[GB_PLANES][NTB];
        load_planes(bn, u_lo * SPU);
        for (int u = u_lo; u < u_hi; ++u) {
            // the unit's bytes into the wave's image (the wave's own reads of the previous unit are complete: DS operations of a wave execute in order)
#pragma unroll
            for (int n = 0; n < NLD; ++n) *reinterpret_cast<u32x4*>(stage + (s_pk[n] & 0xFFFFu)) = wreg[n];
            if (u + 1 < u_hi) load_unit(wreg, u + 1);   // the next unit streams in under this one's steps
            const uint32_t uoff = (uint32_t)u * D::UB;
            typename D::Hdr hdr[RT];
            typename D::MinOp mop[RT];
            const uint8_t* cur[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const uint8_t* first = D::RP ? img[rt] : img[rt] + ((my_row[rt] + uoff) & 15u);
                hdr[rt] = D::header(first, first + 4 * g);
                mop[rt] = D::min_operand(hdr[rt], g);
                cur[rt] = D::RP ? first : (AL ? img[rt] + ((my_row[rt] + uoff) & 12u) : first);
            }
            // the step sums of the unit (K-quant minimum term): 8 bytes per lane, plane and token block
            uint64_t sv[GB_PLANES][NTB];
            if constexpr (D::HAS_MIN) {
#pragma unroll
                for (int pl = 0; pl < GB_PLANES; ++pl)
#pragma unroll
                    for (int tb = 0; tb < NTB; ++tb)
                        sv[pl][tb] = *reinterpret_cast<const uint64_t*>(p.aux + (size_t)u * GB_MIN_UNIT_BYTES + pl * (GB_MIN_UNIT_BYTES / 2) + ((tb * 2 + (g & 1)) * 16 + i) * 8);
            }
#pragma unroll
            for (int j = 0; j < SPU; ++j) {
                u32x4 b[GB_PLANES][NTB];
#pragma unroll
                for (int pl = 0; pl < GB_PLANES; ++pl)
#pragma unroll
                    for (int tb = 0; tb < NTB; ++tb) b[pl][tb] = bn[pl][tb];
                const int nxt = u * SPU + j + 1;
                if (nxt < u_hi * SPU) load_planes(bn, nxt);   // (uniform) one step ahead
                AOp a[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) a[rt] = D::template convert<AL>(D::template load<AL>(cur[rt], cur[rt] + 4 * g, hdr[rt], j, u & 1), j, u & 1);
#pragma unroll
                for (int tb = 0; tb < NTB; ++tb) {
                    if constexpr (D::SPLIT16) {
                        f32x4 cl[RT], ch[RT];
#pragma unroll
                        for (int pl = 0; pl < GB_PLANES; ++pl) {
                            const f16x4 xl = __builtin_bit_cast(f16x4, (uint64_t)b[pl][tb].x | ((uint64_t)b[pl][tb].y << 32));
                            const f16x4 xh = __builtin_bit_cast(f16x4, (uint64_t)b[pl][tb].z | ((uint64_t)b[pl][tb].w << 32));
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt) {
                                const f16x4 wl = __builtin_bit_cast(f16x4, (uint64_t)a[rt].a.x | ((uint64_t)a[rt].a.y << 32));
                                const f16x4 wh = __builtin_bit_cast(f16x4, (uint64_t)a[rt].a.z | ((uint64_t)a[rt].a.w << 32));
                                const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                                cl[rt] = __builtin_amdgcn_mfma_f32_16x16x16f16(xl, wl, pl ? cl[rt] : z, 0, 0, 0);
                                ch[rt] = __builtin_amdgcn_mfma_f32_16x16x16f16(xh, wh, pl ? ch[rt] : z, 0, 0, 0);
                            }
                        }
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[rt][tb][e] = fmaf(a[rt].s1, ch[rt][e], fmaf(a[rt].s0, cl[rt][e], acc[rt][tb][e]));
                    } else {
                        f32x4 cc[RT];
#pragma unroll
                        for (int pl = 0; pl < GB_PLANES; ++pl)
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt) {
                                const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                                cc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, b[pl][tb]), __builtin_bit_cast(f16x8, a[rt].a), pl ? cc[rt] : z, 0, 0, 0);
                            }
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[rt][tb][e] = fmaf(a[rt].s0, cc[rt][e], acc[rt][tb][e]);
                    }
                }
            }
            if constexpr (D::HAS_MIN) {   // - dmin sum_j m_j S_j of the unit (the kernel above: one K = 8 product per (row, token))
#pragma unroll
                for (int tb = 0; tb < NTB; ++tb) {
                    f32x4 rr[RT];
#pragma unroll
                    for (int pl = 0; pl < GB_PLANES; ++pl) {
                        const u32x4 sa = {(uint32_t)sv[pl][tb], (uint32_t)(sv[pl][tb] >> 32), (uint32_t)sv[pl][tb], (uint32_t)(sv[pl][tb] >> 32)};
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) {
                            const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                            const u32x4 mb = {mop[rt].m0, mop[rt].m1, 0u, 0u};
                            rr[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, sa), __builtin_bit_cast(f16x8, mb), pl ? rr[rt] : z, 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[rt][tb][e] = fmaf(mop[rt].ndmin64, rr[rt][e], acc[rt][tb][e]);
                }
            }
        }
    }
    // ---- the waves' partial sums: [wave][rt][tb][lane] float4 in LDS, added in wave order by the waves that store ----
    f32x4* part = reinterpret_cast<f32x4*>(gs_lds + (size_t)NW * (ROWS * STRIDE));
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int tb = 0; tb < NTB; ++tb) part[((size_t)wave * RT * NTB + rt * NTB + tb) * 64 + lane] = acc[rt][tb];
    __syncthreads();
    for (int q = wave; q < RT * NTB; q += NW) {   // (rt, tb) pairs go round the waves
        const int rt = q / NTB, tb = q - rt * NTB;
        f32x4 v = part[(size_t)q * 64 + lane];
        for (int w = 1; w < NW; ++w) {
            const f32x4 t = part[((size_t)w * RT * NTB + q) * 64 + lane];
            v[0] += t[0]; v[1] += t[1]; v[2] += t[2]; v[3] += t[3];
        }
        const int r = row0 + rt * 16 + i;
        if (r >= seg_out) continue;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int t = tb * 16 + 4 * g + e;
            if (t < p.T) {
                const size_t at = (size_t)t * seg_out + r;
                const float y = v[e] * p.inv[t];
                p.seg[sidx].Y[at] = p.resid ? y + p.resid[at] : y;
            }
        }
    }
}

// ---- short prompts, second form (round 6, late): K-SLICE-stationary -- the activation planes of a K slice live in LDS, the weights stream past them ------------
// What bounded the form above was not latency but the planes' own traffic: every wave fetches the 2 KiB (x NTB) of planes of every step it multiplies from
// L2, 3.8 x the weight bytes of a 16-row tile -- Wo of the 8B model at 16 tokens: 17.8 MB of weights and 67 MB of planes per launch, and (weights + planes) /
// time came out at 6.5 - 8 TB/s for every projection, i.e. the L2 -> CU path, with every workgroup of an XCD asking the same channels for the same lines.
// (A request queue in consumption order -- weights and planes the same distance ahead -- changed nothing: profiles/r06_prompt_kslice.txt.)
// Here a workgroup owns a K SLICE (blockIdx.y) and NW row tiles: the slice's planes are copied ONCE into LDS by LDS-DMA (<= 64 / NTB steps = 128 KB), every
// wave then streams ITS tile's weights of the slice (loader, per-wave image and decoders as above, DEPTH units of weights in flight per wave in registers)
// and reads the B operands of a step from LDS.  Planes traffic = slice bytes per workgroup (Wo: 8 MB instead of 67); the slices' partial sums go to the
// partial-sum area the K splits of the large kernel use ([slice][token][row]; summed in slice order by the launch that consumes the projection or by
// reduce_splits_kernel), a launch with ONE slice writes Y itself.
struct GemmKParams {
    GemmBSeg seg[GB_MAX_SEG];
    int nseg;
    const uint8_t* xb;      // operand planes of the (single) chunk
    const uint8_t* aux;     // its step sums (K-quant minimum term)
    const float* inv;       // [T]: 1 / s
    const float* resid;     // (one slice only)
    int T, in, steps;
    unsigned row_bytes;
    int nsplit, units_per_split;   // blockIdx.y = K slice of units_per_split units (a multiple of the ring depth; nsplit * units_per_split = all units)
    int tiles;                     // row tiles (16 RT rows) of all matrices; (blockIdx.x + job * gridDim.x) * NW + wave = this wave's in job `job`
    int jobs;                      // row groups per workgroup
};

template <int DT, int RT, int NTB, bool AL>
__global__ __launch_bounds__((64 * gk_waves<DT, RT, NTB>())) void gemm_quant_f16_kslice_kernel(const GemmKParams p) {
    using D = DeqI<DT>;
    constexpr int SPU = D::SPU, NCH = D::NCH, STRIDE = D::STRIDE;
    constexpr int ROWS = 16 * RT, PIECES = D::RP ? RT * D::PPI : ROWS * NCH, NLD = (PIECES + 63) / 64;
    constexpr int DEPTH = gk_depth<SPU>();
    extern __shared__ __attribute__((aligned(16))) uint8_t gk_lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), NW = (int)(blockDim.x >> 6);
    const int i = lane & 15, g = lane >> 4;
    // the slice
    const int U = p.steps / SPU;
    const int u_lo = (int)blockIdx.y * p.units_per_split, u_hi = min(u_lo + p.units_per_split, U);
    const int nrec = (u_hi - u_lo) * SPU * GB_PLANES * NTB;   // 1 KiB records (step, piece, token block) of the slice
    const uint32_t planes_bytes = (uint32_t)p.units_per_split * SPU * GB_PLANES * NTB * GB_PIECE;
    // ---- the slice's planes: LDS-DMA, 1 KiB per wave request, ONCE per workgroup -- for all the row groups it takes (p.jobs of them, gridDim.x apart:
    // the planner folds what would be a second and third round of workgroups over the 256 CUs into the first, so that a CU copies a slice's planes
    // once; counters of the form without it: 1.5 x the weight bytes fetched past L2 on the long launches, profiles/r06_prompt_kslice_pmc_8b_q8_0.txt) ----
    {
        const uint32_t lds0 = (uint32_t)(uintptr_t)gk_lds;   // (LDS address = the low 32 bits of the generic pointer's offset: see gb_dma16's callers above)
        const uint8_t* src0 = p.xb + (size_t)u_lo * SPU * GB_STEP_BYTES + (size_t)lane * 16;
        for (int r = wave; r < nrec; r += NW) {
            const int s = r / (GB_PLANES * NTB), q = r - s * (GB_PLANES * NTB), pl = q / NTB, tb = q - pl * NTB;
            gb_dma16(__builtin_amdgcn_readfirstlane(lds0 + (uint32_t)r * GB_PIECE), src0 + (size_t)s * GB_STEP_BYTES + (size_t)(pl * 4 + tb) * GB_PIECE);
        }
    }
    for (int it = 0; it < p.jobs; ++it) {
    // this wave's tile (waves past the last tile only help with the copy)
    const int tile_raw = ((int)blockIdx.x + it * (int)gridDim.x) * NW + wave;
    const int tile = min(tile_raw, p.tiles - 1);
    const bool has_tile = tile_raw < p.tiles;
    int sidx = 0;
    if (p.nseg > 1 && tile >= p.seg[1].tile0) sidx = 1;
    if (p.nseg > 2 && tile >= p.seg[2].tile0) sidx = 2;
    const uint8_t* const segW = p.seg[sidx].W;
    const int seg_out = p.seg[sidx].out;
    const unsigned seg_w_last = p.seg[sidx].w_last;
    const int row0 = (tile - p.seg[sidx].tile0) * ROWS;
    uint8_t* stage = gk_lds + planes_bytes + (size_t)wave * (ROWS * STRIDE);
    uint32_t w_row[NLD], s_pk[NLD];
    if constexpr (D::RP) {
        const unsigned nsb = (unsigned)(p.in / 256);
#pragma unroll
        for (int n = 0; n < NLD; ++n) {
            const int q = min(64 * n + lane, PIECES - 1), rt = q / D::PPI, idx = q - rt * D::PPI;
            const unsigned t16 = (unsigned)min(row0 / 16 + rt, p.seg[sidx].tiles16 - 1);
            const bool rec = idx >= 2 * D::S1 / 16;
            w_row[n] = rec ? p.seg[sidx].p2_off + t16 * nsb * (unsigned)D::S2 + 16u * (unsigned)(idx - 2 * D::S1 / 16) : t16 * nsb * (unsigned)(2 * D::S1) + 16u * (unsigned)idx;
            s_pk[n] = (uint32_t)(rt * D::ITEM + 16 * idx) | ((uint32_t)(rec ? D::S2 : 2 * D::S1) << 16);
        }
    } else {
#pragma unroll
        for (int n = 0; n < NLD; ++n) {
            const int q = min(64 * n + lane, PIECES - 1), r = q / NCH, c = q - r * NCH;
            w_row[n] = (uint32_t)min(row0 + r, seg_out - 1) * p.row_bytes;
            s_pk[n] = (uint32_t)(r * STRIDE + 16 * c) | ((uint32_t)(16 * c) << 16);
        }
    }
    auto load_unit = [&](u32x4 (&w)[NLD], int unit) {
#pragma unroll
        for (int n = 0; n < NLD; ++n) {
            uint32_t off;
            if constexpr (D::RP) off = w_row[n] + (uint32_t)unit * (s_pk[n] >> 16);
            else off = min(((w_row[n] + (uint32_t)unit * D::UB) & ~15u) + (s_pk[n] >> 16), seg_w_last);
            w[n] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(segW + off));
        }
    };
    auto load_sums = [&](uint64_t (&v)[GB_PLANES][NTB], int unit) {   // the step sums of a unit (K-quant minimum term): 8 bytes per lane, piece and token block
#pragma unroll
        for (int pl = 0; pl < GB_PLANES; ++pl)
#pragma unroll
            for (int tb = 0; tb < NTB; ++tb)
                v[pl][tb] = *reinterpret_cast<const uint64_t*>(p.aux + (size_t)unit * GB_MIN_UNIT_BYTES + pl * (GB_MIN_UNIT_BYTES / 2) + ((tb * 2 + (g & 1)) * 16 + i) * 8);
    };
    const uint8_t* img[RT];
    uint32_t my_row[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        img[rt] = D::RP ? stage + rt * D::ITEM + 16 * i : stage + (rt * 16 + i) * STRIDE;
        my_row[rt] = (uint32_t)min(row0 + rt * 16 + i, seg_out - 1) * p.row_bytes;
    }
    f32x4 acc[RT][NTB];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int tb = 0; tb < NTB; ++tb) acc[rt][tb] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    // ---- prologue of a row group: its first DEPTH units of weights go out (HBM: the long round trip; for the first group, behind the planes' copy) ----
    // (scheduling barriers between the requests: the compiler counts its waits from their ORDER -- shuffled, it ends in vmcnt(0) at the head of every group)
    u32x4 wreg[DEPTH][NLD];
    uint64_t svr[D::HAS_MIN ? DEPTH : 1][GB_PLANES][NTB];
    const int u_last = u_hi - 1;
#pragma unroll
    for (int k = 0; k < DEPTH; ++k) {   // (requests past the slice repeat its last unit: straight-line code, exact waits)
        load_unit(wreg[k], min(u_lo + k, u_last));
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (D::HAS_MIN) { load_sums(svr[k], min(u_lo + k, u_last)); __builtin_amdgcn_sched_barrier(0); }
    }
    if (it == 0) {   // (uniform) the planes have landed -- and with them this job's first weights; later jobs find the planes there
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the compiler does not count the DMAs)
        __syncthreads();
    }
    const u32x4* planes = reinterpret_cast<const u32x4*>(gk_lds) + lane;   // + ((local step * GB_PLANES + piece) * NTB + token block) * 64
    if (has_tile) {
        // Groups of DEPTH units, no exit inside (the ring registers never move); every slice is a whole number of groups -- the host plans no other
        // slices.  (A first build let a short last group run its requests and image writes with the arithmetic skipped: the image writes of such idle
        // units -- the SAME bytes again -- made whole tiles of other waves come out wrong, differently from launch to launch, with every wait in place
        // (profiles/r06_prompt_kslice.txt); unexplained, and avoided: nothing is ever written to an image that is not multiplied afterwards.)
        for (int ug = u_lo; ug < u_hi; ug += DEPTH) {
#pragma unroll
        for (int k = 0; k < DEPTH; ++k) {
            const int u = ug + k;
            // the unit's bytes into the wave's image (the wave's own reads of the previous unit are complete: DS operations of a wave execute in order)
#pragma unroll
            for (int n = 0; n < NLD; ++n) *reinterpret_cast<u32x4*>(stage + (s_pk[n] & 0xFFFFu)) = wreg[k][n];
            const int u_next = min(u + DEPTH, u_last);
            __builtin_amdgcn_sched_barrier(0);
            load_unit(wreg[k], u_next);
            __builtin_amdgcn_sched_barrier(0);
            uint64_t sv[GB_PLANES][NTB];
            if constexpr (D::HAS_MIN) {
#pragma unroll
                for (int pl = 0; pl < GB_PLANES; ++pl)
#pragma unroll
                    for (int tb = 0; tb < NTB; ++tb) sv[pl][tb] = svr[k][pl][tb];
                __builtin_amdgcn_sched_barrier(0);
                load_sums(svr[k], u_next);   // (same queue, same distance, consumption order: behind the unit's weights)
                __builtin_amdgcn_sched_barrier(0);
            }
            const uint32_t uoff = (uint32_t)u * D::UB;
            typename D::Hdr hdr[RT];
            typename D::MinOp mop[RT];
            const uint8_t* cur[RT];
#pragma unroll
            for (int rt = 0; rt < RT; ++rt) {
                const uint8_t* first = D::RP ? img[rt] : img[rt] + ((my_row[rt] + uoff) & 15u);
                hdr[rt] = D::header(first, first + 4 * g);
                mop[rt] = D::min_operand(hdr[rt], g);
                cur[rt] = D::RP ? first : (AL ? img[rt] + ((my_row[rt] + uoff) & 12u) : first);
            }
            const u32x4* pu = planes + (size_t)(u - u_lo) * SPU * (GB_PLANES * NTB * 64);
#pragma unroll
            for (int j = 0; j < SPU; ++j) {
                u32x4 b[GB_PLANES][NTB];
#pragma unroll
                for (int pl = 0; pl < GB_PLANES; ++pl)
#pragma unroll
                    for (int tb = 0; tb < NTB; ++tb) b[pl][tb] = pu[((j * GB_PLANES + pl) * NTB + tb) * 64];
                AOp a[RT];
#pragma unroll
                for (int rt = 0; rt < RT; ++rt) a[rt] = D::template convert<AL>(D::template load<AL>(cur[rt], cur[rt] + 4 * g, hdr[rt], j, u & 1), j, u & 1);
#pragma unroll
                for (int tb = 0; tb < NTB; ++tb) {
                    if constexpr (D::SPLIT16) {
                        f32x4 cl[RT], ch[RT];
#pragma unroll
                        for (int pl = 0; pl < GB_PLANES; ++pl) {
                            const f16x4 xl = __builtin_bit_cast(f16x4, (uint64_t)b[pl][tb].x | ((uint64_t)b[pl][tb].y << 32));
                            const f16x4 xh = __builtin_bit_cast(f16x4, (uint64_t)b[pl][tb].z | ((uint64_t)b[pl][tb].w << 32));
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt) {
                                const f16x4 wl = __builtin_bit_cast(f16x4, (uint64_t)a[rt].a.x | ((uint64_t)a[rt].a.y << 32));
                                const f16x4 wh = __builtin_bit_cast(f16x4, (uint64_t)a[rt].a.z | ((uint64_t)a[rt].a.w << 32));
                                const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                                cl[rt] = __builtin_amdgcn_mfma_f32_16x16x16f16(xl, wl, pl ? cl[rt] : z, 0, 0, 0);
                                ch[rt] = __builtin_amdgcn_mfma_f32_16x16x16f16(xh, wh, pl ? ch[rt] : z, 0, 0, 0);
                            }
                        }
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[rt][tb][e] = fmaf(a[rt].s1, ch[rt][e], fmaf(a[rt].s0, cl[rt][e], acc[rt][tb][e]));
                    } else {
                        f32x4 cc[RT];
#pragma unroll
                        for (int pl = 0; pl < GB_PLANES; ++pl)
#pragma unroll
                            for (int rt = 0; rt < RT; ++rt) {
                                const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                                cc[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, b[pl][tb]), __builtin_bit_cast(f16x8, a[rt].a), pl ? cc[rt] : z, 0, 0, 0);
                            }
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[rt][tb][e] = fmaf(a[rt].s0, cc[rt][e], acc[rt][tb][e]);
                    }
                }
            }
            if constexpr (D::HAS_MIN) {   // - dmin sum_j m_j S_j of the unit (the large kernel: one K = 8 product per (row, token))
#pragma unroll
                for (int tb = 0; tb < NTB; ++tb) {
                    f32x4 rr[RT];
#pragma unroll
                    for (int pl = 0; pl < GB_PLANES; ++pl) {
                        const u32x4 sa = {(uint32_t)sv[pl][tb], (uint32_t)(sv[pl][tb] >> 32), (uint32_t)sv[pl][tb], (uint32_t)(sv[pl][tb] >> 32)};
#pragma unroll
                        for (int rt = 0; rt < RT; ++rt) {
                            const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
                            const u32x4 mb = {mop[rt].m0, mop[rt].m1, 0u, 0u};
                            rr[rt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, sa), __builtin_bit_cast(f16x8, mb), pl ? rr[rt] : z, 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
                        for (int e = 0; e < 4; ++e) acc[rt][tb][e] = fmaf(mop[rt].ndmin64, rr[rt][e], acc[rt][tb][e]);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        }
        // ---- this wave's rows: accumulator element e of lane (i = row of the tile, g) is token tb * 16 + 4 g + e; 1 / s; Y or this slice's partial sums ----
        f32x4 inv_t[NTB];
#pragma unroll
        for (int tb = 0; tb < NTB; ++tb) inv_t[tb] = *reinterpret_cast<const f32x4*>(p.inv + tb * 16 + 4 * g);   // (the array is padded to whole chunks)
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
            const int r = row0 + rt * 16 + i;
            if (r >= seg_out) continue;
#pragma unroll
            for (int tb = 0; tb < NTB; ++tb)
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int t = tb * 16 + 4 * g + e;
                    if (t >= p.T) continue;
                    const float y = acc[rt][tb][e] * inv_t[tb][e];
                    if (p.nsplit > 1) p.seg[sidx].part[((size_t)blockIdx.y * p.T + t) * seg_out + r] = y;
                    else { const size_t at = (size_t)t * seg_out + r; p.seg[sidx].Y[at] = p.resid ? y + p.resid[at] : y; }
                }
        }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // (the ring's last requests: nothing may be in flight when the wave moves on or retires)
    }
}

// Y[t][r] = sum over splits (in order) of part[s][t][r] (+ resid): one float4 per thread, blockIdx.y = matrix of the launch
struct ReduceArgs {
    float* Y[GB_MAX_SEG];
    const float* part[GB_MAX_SEG];
    int out[GB_MAX_SEG];
    const float* resid;
    int nseg, T, nsplit;
};
__global__ __launch_bounds__(256) void reduce_splits_kernel(const ReduceArgs a) {
    const int sg = blockIdx.y;
    float* Y = a.Y[0];
    const float* part = a.part[0];
    int out = a.out[0];
    if (sg == 1) { Y = a.Y[1]; part = a.part[1]; out = a.out[1]; }
    if (sg == 2) { Y = a.Y[2]; part = a.part[2]; out = a.out[2]; }
    const size_t idx = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (idx >= (size_t)a.T * out) return;
    float4 v = *reinterpret_cast<const float4*>(part + idx);
    for (int s = 1; s < a.nsplit; ++s) {
        const float4 q = *reinterpret_cast<const float4*>(part + (size_t)s * a.T * out + idx);
        v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    if (a.resid) {
        const float4 q = *reinterpret_cast<const float4*>(a.resid + idx);
        v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
    }
    *reinterpret_cast<float4*>(Y + idx) = v;
}

// ---- the K splits' sums folded into the launch that consumes the projection (the reduce launch deferred: ntk_gemm_partials) ---------
// hidden[t] = (part[0][t] + part[1][t] + ...) + hidden[t]   (reduce_splits_kernel's order, the residual last), then RMSNorm of the new row into
// x_out + the row's largest |x| (rmsnorm_rowmax_kernel's expressions, sums and block size: identical bits).  One workgroup per token.
__global__ __launch_bounds__(1024) void reduce_rmsnorm_rowmax_kernel(float* __restrict__ hidden, const float* __restrict__ part, int nsplit, int T, int H,
                                                                     const float* __restrict__ weight, float eps, float* __restrict__ x_out,
                                                                     float* __restrict__ row_max, float* __restrict__ zero, uint8_t* __restrict__ ws) {
    __shared__ float red[16];
    if ((int)blockIdx.x >= T) { split_row(nullptr, 0u, (int)blockIdx.x, H, ws); return; }   // (ws launches only: the padding tokens' zero records)
    const size_t row = (size_t)blockIdx.x * H, plane = (size_t)T * H;
    float* h = hidden + row;
    const int bd = (int)blockDim.x, tid = (int)threadIdx.x;
    float ssq = 0.0f;
    // the thread's elements tid, tid + bd, ... (rmsnorm_kernel's assignment and accumulation order), eight at a time, the splits four at a time:
    // 32 independent loads in flight, the additions in split order (a rolled loop over the splits is one dependent load per addition:
    // 20 us per launch at 64 tokens x 8 splits, profiles/r05_prefill_row_max_ab.txt)
    for (int i0 = tid; i0 < H; i0 += 8 * bd) {
        int idx[8];
        float v[8], r[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) idx[k] = min(i0 + k * bd, H - 1);
#pragma unroll
        for (int k = 0; k < 8; ++k) { v[k] = part[row + idx[k]]; r[k] = h[idx[k]]; }
        for (int sp = 1; sp < nsplit; sp += 4) {
            float q[4][8];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const size_t at = (size_t)min(sp + j, nsplit - 1) * plane + row;
#pragma unroll
                for (int k = 0; k < 8; ++k) q[j][k] = part[at + idx[k]];
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (sp + j < nsplit) {   // (uniform)
#pragma unroll
                    for (int k = 0; k < 8; ++k) v[k] += q[j][k];
                }
        }
#pragma unroll
        for (int k = 0; k < 8; ++k)
            if (i0 + k * bd < H) {
                const float y = v[k] + r[k];
                h[i0 + k * bd] = y;
                ssq = fmaf(y, y, ssq);
            }
    }
    const float tot = block_sum(ssq, red);
    const float rms_inv = 1.0f / sqrtf(tot / (float)H + eps);
    uint32_t mb = 0;
    for (int i = tid; i < H; i += bd) {   // (h[i]: this thread's own stores)
        const float v = h[i] * rms_inv * weight[i];
        x_out[row + i] = v;
        mb = max(mb, __float_as_uint(v) & 0x7FFFFFFFu);
    }
    const float m = block_max(__uint_as_float(mb <= 0x7F800000u ? mb : 0x7F800000u), red);
    if (ws) {   // the row this workgroup has written, split for the projection that follows (reuse_x = 1)
        __syncthreads();
        split_row(x_out + row, __float_as_uint(m), (int)blockIdx.x, H, ws);
        return;
    }
    if (tid == 0) {
        row_max[blockIdx.x] = m;
        if (zero) zero[blockIdx.x] = 0.0f;
    }
}
// out = silu(gate) * up (the sums of their K splits, in split order, when nsplit > 1) -- silu_mul_rowmax_kernel's / reduce_silu_mul_rowmax_kernel's
// expressions -- by ONE workgroup per token, which then splits the row it has written for the down projection.  pg / pu: [nsplit][T][I] (nsplit = 1: the
// projections' outputs themselves).
__global__ __launch_bounds__(1024) void silu_mul_split_kernel(float* out, const float* pg, const float* pu, int nsplit,
                                                              int T, int I, uint8_t* __restrict__ ws) {
    __shared__ float red[16];
    const int t = (int)blockIdx.x;
    if (t >= T) { split_row(nullptr, 0u, t, I, ws); return; }
    const size_t plane = (size_t)T * I;
    uint32_t mb = 0;
    for (int i = (int)threadIdx.x * 4; i < I; i += (int)blockDim.x * 4) {
        const size_t at = (size_t)t * I + i;
        float4 g = *reinterpret_cast<const float4*>(pg + at), u = *reinterpret_cast<const float4*>(pu + at);
        for (int sp = 1; sp < nsplit; ++sp) {
            const float4 a = *reinterpret_cast<const float4*>(pg + (size_t)sp * plane + at), b = *reinterpret_cast<const float4*>(pu + (size_t)sp * plane + at);
            g.x += a.x; g.y += a.y; g.z += a.z; g.w += a.w;
            u.x += b.x; u.y += b.y; u.z += b.z; u.w += b.w;
        }
        float4 o;
        o.x = g.x / (1.0f + expf(-g.x)) * u.x; o.y = g.y / (1.0f + expf(-g.y)) * u.y;
        o.z = g.z / (1.0f + expf(-g.z)) * u.z; o.w = g.w / (1.0f + expf(-g.w)) * u.w;
        *reinterpret_cast<float4*>(out + at) = o;
        mb = max(mb, max(max(__float_as_uint(o.x) & 0x7FFFFFFFu, __float_as_uint(o.y) & 0x7FFFFFFFu),
                         max(__float_as_uint(o.z) & 0x7FFFFFFFu, __float_as_uint(o.w) & 0x7FFFFFFFu)));
    }
    const float m = block_max(__uint_as_float(mb <= 0x7F800000u ? mb : 0x7F800000u), red);
    __syncthreads();
    split_row(out + (size_t)t * I, __float_as_uint(m), t, I, ws);
}
// out = silu(sum of gate's splits) * (sum of up's splits) + max |out| per token (silu_mul_rowmax_kernel's expressions).  grid (ceil(I / 1024), T)
__global__ __launch_bounds__(256) void reduce_silu_mul_rowmax_kernel(float* __restrict__ out, const float* __restrict__ pg, const float* __restrict__ pu,
                                                                     int nsplit, int T, int I, float* __restrict__ row_max) {
    __shared__ float red[16];
    const int t = blockIdx.y, i = ((int)blockIdx.x * 256 + (int)threadIdx.x) * 4;
    uint32_t mb = 0;
    if (i < I) {
        const size_t at = (size_t)t * I + i, plane = (size_t)T * I;
        float4 g = *reinterpret_cast<const float4*>(pg + at), u = *reinterpret_cast<const float4*>(pu + at);
        for (int sp = 1; sp < nsplit; ++sp) {
            const float4 a = *reinterpret_cast<const float4*>(pg + (size_t)sp * plane + at), b = *reinterpret_cast<const float4*>(pu + (size_t)sp * plane + at);
            g.x += a.x; g.y += a.y; g.z += a.z; g.w += a.w;
            u.x += b.x; u.y += b.y; u.z += b.z; u.w += b.w;
        }
        float4 o;
        o.x = g.x / (1.0f + expf(-g.x)) * u.x; o.y = g.y / (1.0f + expf(-g.y)) * u.y;
        o.z = g.z / (1.0f + expf(-g.z)) * u.z; o.w = g.w / (1.0f + expf(-g.w)) * u.w;
        *reinterpret_cast<float4*>(out + at) = o;
        mb = max(max(__float_as_uint(o.x) & 0x7FFFFFFFu, __float_as_uint(o.y) & 0x7FFFFFFFu),
                 max(__float_as_uint(o.z) & 0x7FFFFFFFu, __float_as_uint(o.w) & 0x7FFFFFFFu));
    }
    const float m = block_max(__uint_as_float(mb <= 0x7F800000u ? mb : 0x7F800000u), red);
    if (threadIdx.x == 0) atomicMax(reinterpret_cast<unsigned*>(row_max) + t, __float_as_uint(m));
}

struct HostSeg { float* Y; const void* W; int out; };
using I1 = std::integral_constant<int, 1>;
using I2 = std::integral_constant<int, 2>;

// the plan's tuning switches (tuning builds only: the shipping library runs the defaults and reads no environment), read once
static const GemmTune& gemm_tune() {
    static constexpr GemmTune d{};
    static const GemmTune t = [] {
        GemmTune t;
        t.kslice = NTK_TUNE_ENV_INT("NTK_GEMM_KSLICE", d.kslice); t.kslice_jobs = NTK_TUNE_ENV_INT("NTK_GEMM_KSLICE_JOBS", d.kslice_jobs);
        t.kslice_c0 = NTK_TUNE_ENV_INT("NTK_GEMM_KSLICE_C0", d.kslice_c0); t.kslice_c1 = NTK_TUNE_ENV_INT("NTK_GEMM_KSLICE_C1", d.kslice_c1);
        t.kslice_rt = NTK_TUNE_ENV_INT("NTK_GEMM_KSLICE_RT", d.kslice_rt); t.kslice_n = NTK_TUNE_ENV_INT("NTK_GEMM_KSLICE_N", d.kslice_n);
        t.small = NTK_TUNE_ENV_INT("NTK_GEMM_SMALL", d.small); t.small_rt = NTK_TUNE_ENV_INT("NTK_GEMM_SMALL_RT", d.small_rt);
        t.small_nw = NTK_TUNE_ENV_INT("NTK_GEMM_SMALL_NW", d.small_nw); t.map = NTK_TUNE_ENV_INT("NTK_GEMM_MAP", d.map);
        t.rt = NTK_TUNE_ENV_INT("NTK_GEMM_RT", d.rt); t.wgs = NTK_TUNE_ENV_INT("NTK_GEMM_WGS", d.wgs);
        t.no_pf = NTK_TUNE_ENV_INT("NTK_GEMM_NO_PF", d.no_pf); t.cw = NTK_TUNE_ENV_INT("NTK_GEMM_CW", d.cw);
        return t;
    }();
    return t;
}

// what a consumer needs of a launch: nsplit > 1 -- the partial sums are `part`'s and it sums them (and adds the residual) itself; 1 -- Y is written
static void set_partials(ntk_gemm_partials* d, const HostSeg* segs, int nseg, int T, int nsplit, float* const* part) {
    if (!d) return;
    d->nseg = nseg; d->n_tokens = T; d->nsplit = nsplit;
    for (int i = 0; i < nseg; ++i) { d->part[i] = part && nsplit > 1 ? part[i] : nullptr; d->y[i] = segs[i].Y; d->rows[i] = segs[i].out; }
}
static void reduce_splits(const HostSeg* segs, float* const* part, int nseg, int T, int nsplit, const float* resid, hipStream_t st) {
    ReduceArgs ra{};
    ra.nseg = nseg; ra.T = T; ra.nsplit = nsplit; ra.resid = resid;
    size_t biggest = 0;
    for (int i = 0; i < nseg; ++i) {
        ra.Y[i] = segs[i].Y; ra.part[i] = part[i]; ra.out[i] = segs[i].out;
        biggest = std::max(biggest, ((size_t)T * segs[i].out + 3) / 4);
    }
    hipLaunchKernelGGL(reduce_splits_kernel, dim3((unsigned)((biggest + 255) / 256), nseg), dim3(256), 0, st, ra);
}
// what the three parameter structs share: the matrices in the plan's tile numbering, the operand planes, step sums and 1 / s in the workspace
template <class P>
static void fill_params(P& p, const GemmPlan& plan, const HostSeg* segs, int nseg, int T, int in, const float* resid, uint8_t* wsb, float* const* part) {
    p.nseg = nseg; p.T = T; p.in = in; p.steps = in / 32; p.row_bytes = plan.row_bytes;
    p.xb = wsb;
    p.aux = reinterpret_cast<decltype(p.aux)>(wsb + (size_t)(p.steps + 1) * GB_STEP_BYTES);
    p.inv = reinterpret_cast<const float*>(wsb + (size_t)GB_MAX_CHUNKS * ws_chunk_bytes(in));   // [inv: 1024][scale: 1024]
    p.resid = resid;
    for (int i = 0; i < nseg; ++i) {
        GemmBSeg& s = p.seg[i];
        s.W = static_cast<const uint8_t*>(segs[i].W); s.Y = segs[i].Y; s.part = part[i]; s.out = segs[i].out;
        s.tile0 = plan.seg[i].tile0; s.tiles16 = plan.seg[i].tiles16; s.w_last = plan.seg[i].w_last; s.p2_off = plan.seg[i].p2_off;
    }
}

// The instantiations of each form, visited with their template arguments as constants: the LDS opt-in visits them all, a launch runs the one its plan names.
template <bool SKIP22, class F> static void each_rt_ntb_al(F f) {   // the short forms: RT x NTB x AL
    auto both = [&](auto rt, auto ntb) {
        if constexpr (!(SKIP22 && decltype(rt)::value == 2 && decltype(ntb)::value == 2)) { f(rt, ntb, std::true_type{}); f(rt, ntb, std::false_type{}); }
    };
    both(I1{}, I1{}); both(I2{}, I1{}); both(I1{}, I2{}); both(I2{}, I2{});
}
template <int DT, class F> static void each_chunk_kernel(F f) {   // the chunk form: RT x AL x PF x CW
    using PFD = std::bool_constant<DeqI<DT>::PF>; using Y = std::true_type; using N = std::false_type;
    f(I2{}, Y{}, PFD{}, I1{}); f(I2{}, N{}, PFD{}, I1{}); f(I1{}, Y{}, PFD{}, I1{}); f(I1{}, N{}, PFD{}, I1{});
    if constexpr (PFD::value) { f(I2{}, Y{}, N{}, I1{}); f(I1{}, Y{}, N{}, I1{}); }   // (without the plane prefetch: aligned rows only)
    if constexpr (gb_cw2_ok<DT>()) f(I2{}, Y{}, N{}, I2{});
}

// visit(f) calls f(kernel, the most dynamic LDS it can be launched with, whether it is the plan's) for every instantiation of a form: each opts in to its
// LDS (more than 64 KB, up to 160) once, and the plan's is launched
template <class P, class V> static int launch_form(const GemmPlan& plan, const P& params, hipStream_t st, V visit) {
    static const bool lds_ok = [&] {
        bool ok = true;
        visit([&](auto* k, size_t lds, bool) { ok &= hipFuncSetAttribute(reinterpret_cast<const void*>(k), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) == hipSuccess; });
        return ok;
    }();
    if (!lds_ok) return NTK_E_LAUNCH;
    visit([&](auto* k, size_t, bool mine) { if (mine) hipLaunchKernelGGL(k, dim3(plan.grid_x, plan.grid_y), dim3(plan.block), plan.lds, st, params); });
    return NTK_OK;
}

// T <= GB_MAX_CHUNKS * 64 = 1024 tokens in one launch; nseg matrices [out_s][in] of one format sharing X: the plan (gemm_f16_plan.h: form, tiles, K
// slices, grid), the operand pre-pass, the form's kernel, and the sum of the K slices -- here, or left to the launch that consumes the projection
template <int DT>
static int launch_gemm_f16(const HostSeg* segs, int nseg, const float* X, int T, int in, const float* resid, void* ws, int reuse_x,
                            const float* row_max, ntk_gemm_partials* defer, bool full_form, hipStream_t st) {
    if (nseg < 1 || nseg > GB_MAX_SEG || (resid && nseg != 1)) return NTK_E_SHAPE;
    int rows[GB_MAX_SEG];
    for (int i = 0; i < nseg; ++i) rows[i] = segs[i].out;
    const GemmPlan plan = gemm_f16_plan<DT>(rows, nseg, T, in, full_form, gemm_tune());
    if (plan.status != NTK_OK) return plan.status;
    for (int i = 0; i < nseg; ++i)
        if ((reinterpret_cast<uintptr_t>(segs[i].W) & 15) || (reinterpret_cast<uintptr_t>(segs[i].Y) & 15)) return NTK_E_ALIGN;
    if ((reinterpret_cast<uintptr_t>(X) & 15) || (resid && (reinterpret_cast<uintptr_t>(resid) & 15))) return NTK_E_ALIGN;
    // ---- the operand pre-pass into the workspace: [chunk][planes | sums], [1 / s][s], then the partial sums of the K slices ----
    uint8_t* wsb = static_cast<uint8_t*>(ws);
    const int steps = in / 32, chunks = (T + GB_TOK - 1) / GB_TOK;
    const size_t chunk_bytes = ws_chunk_bytes(in);
    float* aux = reinterpret_cast<float*>(wsb + (size_t)(steps + 1) * GB_STEP_BYTES);
    float* scales = reinterpret_cast<float*>(wsb + (size_t)GB_MAX_CHUNKS * chunk_bytes);   // [inv: 1024][scale: 1024]
    if (!reuse_x && row_max) {   // the tokens' largest |x| came with X: one pre-pass launch
        hipLaunchKernelGGL(split_x_kernel<true>, dim3(steps + 8, chunks), dim3(256), 0, st, X, T, in, reinterpret_cast<u32x4*>(wsb), aux, chunk_bytes, row_max, scales);
    } else if (!reuse_x) {
        hipLaunchKernelGGL(row_scale_kernel, dim3((T + 3) / 4), dim3(256), 0, st, X, T, in, scales + GB_MAX_CHUNKS * GB_TOK, scales);
        hipLaunchKernelGGL(split_x_kernel<false>, dim3(steps + 8, chunks), dim3(256), 0, st, X, T, in, reinterpret_cast<u32x4*>(wsb), aux, chunk_bytes,
                           scales + GB_MAX_CHUNKS * GB_TOK, static_cast<float*>(nullptr));
    }
    float* part[GB_MAX_SEG] = {};   // (the small form splits K over its waves: no partial sums)
    if (plan.form != GEMM_FORM_SMALL)
        for (int i = 0; i < nseg; ++i) part[i] = reinterpret_cast<float*>(wsb + (size_t)GB_MAX_CHUNKS * chunk_bytes + GB_SCALE_BYTES) + plan.seg[i].part_off;
    int rc;
    if (plan.form == GEMM_FORM_KSLICE) {
        GemmKParams kp{};
        fill_params(kp, plan, segs, nseg, T, in, plan.nsplit == 1 ? resid : nullptr, wsb, part);
        kp.nsplit = plan.nsplit; kp.units_per_split = plan.per_split; kp.tiles = plan.tiles; kp.jobs = plan.jobs;
        rc = launch_form(plan, kp, st, [&](auto f) {   // (32 rows x 32 tokens of the format that scales per 16 columns: over the register budget, never planned)
            each_rt_ntb_al<DeqI<DT>::SPLIT16>([&](auto rt, auto ntb, auto al) {
                constexpr int R = decltype(rt)::value, N = decltype(ntb)::value; constexpr bool A = decltype(al)::value;
                f(&gemm_quant_f16_kslice_kernel<DT, R, N, A>, gk_lds_bytes<DT, R, N>(gk_waves<DT, R, N>(), gk_max_steps<DT, R, N>()), R == plan.rt && N == plan.ntb && A == plan.al);
            });
        });
    } else if (plan.form == GEMM_FORM_SMALL) {
        GemmSParams sp{};
        fill_params(sp, plan, segs, nseg, T, in, resid, wsb, part);
        rc = launch_form(plan, sp, st, [&](auto f) {   // (8 waves x (32-row image + partial sums) can exceed 64 KB)
            each_rt_ntb_al<false>([&](auto rt, auto ntb, auto al) {
                constexpr int R = decltype(rt)::value, N = decltype(ntb)::value; constexpr bool A = decltype(al)::value;
                f(&gemm_quant_f16_small_kernel<DT, R, N, A>, gs_lds_bytes<DT, R, N>(8), (R == 2) == (plan.rt == 2) && N == plan.ntb && A == plan.al);
            });
        });
    } else {
        GemmBParams p{};
        fill_params(p, plan, segs, nseg, T, in, resid, wsb, part);
        p.chunks = plan.chunks; p.chunk_bytes = chunk_bytes; p.row_wgs = plan.tiles; p.map8 = gemm_tune().map;
        p.nsplit = plan.nsplit; p.steps_per_split = plan.per_split;
        rc = launch_form(plan, p, st, [&](auto f) {
            each_chunk_kernel<DT>([&](auto rt, auto al, auto pf, auto cw) {
                constexpr int R = decltype(rt)::value, C = decltype(cw)::value; constexpr bool A = decltype(al)::value, PF = decltype(pf)::value;
                f(&gemm_quant_f16_kernel<DT, R, A, PF, C>, gb_lds_bytes<DT, R, C>(), R == plan.rt && A == plan.al && PF == plan.pf && C == plan.cw);
            });
        });
    }
    if (rc != NTK_OK) return rc;
    set_partials(defer, segs, nseg, T, plan.nsplit, part);
    if (plan.nsplit > 1 && !defer) reduce_splits(segs, part, nseg, T, plan.nsplit, resid, st);
    return last_launch_status();
}

// f(std::integral_constant<int, DT>{}) for the format of a call (weight_dtype + GB_RP: the matrices are tensors of the engine's decode repack)
template <class F> static int with_gemm_format(int weight_dtype, F f) {
    switch (weight_dtype) {
        case NTK_DT_Q8_0: return f(std::integral_constant<int, NTK_DT_Q8_0>{});
        case NTK_DT_Q4_0: return f(std::integral_constant<int, NTK_DT_Q4_0>{});
        case NTK_DT_Q4_K: return f(std::integral_constant<int, NTK_DT_Q4_K>{});
        case NTK_DT_Q5_K: return f(std::integral_constant<int, NTK_DT_Q5_K>{});
        case NTK_DT_Q4_K + GB_RP: return f(std::integral_constant<int, NTK_DT_Q4_K + GB_RP>{});
        case NTK_DT_Q5_K + GB_RP: return f(std::integral_constant<int, NTK_DT_Q5_K + GB_RP>{});
        case NTK_DT_Q6_K + GB_RP: return f(std::integral_constant<int, NTK_DT_Q6_K + GB_RP>{});
        default: return f(std::integral_constant<int, NTK_DT_Q6_K>{});
    }
}

}  // namespace ntk

extern "C" {

#ifdef NTK_GEMM_TRACE
__attribute__((visibility("default"))) int ntk_debug_gemm_f16_trace(unsigned long long* out, size_t n) {   // n <= 4 * GBT_STEPS * GBT_EV
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ntk::g_gemm_f16_trace), n * sizeof(unsigned long long)) == hipSuccess ? 0 : -3;
}
__attribute__((visibility("default"))) int ntk_debug_gemm_f16_clock(unsigned long long* out) {   // 4 values
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ntk::g_gemm_f16_clock), 4 * sizeof(unsigned long long)) == hipSuccess ? 0 : -3;
}
#endif

size_t ntk_gemm_quant_workspace_bytes(int in_features, int out_features) {
    if (in_features <= 0 || out_features < 0) return 0;
    return (size_t)ntk::GB_MAX_CHUNKS * ntk::ws_chunk_bytes((in_features + 31) / 32 * 32) + ntk::GB_SCALE_BYTES +
           (size_t)ntk::gb_split_rows(out_features) * ntk::GB_TOK * (size_t)out_features * sizeof(float) + 256;
}

static int gemm_ws_dispatch(const ntk::HostSeg* segs, int nseg, const float* X, int n_tokens, int in_features, int weight_dtype, const float* resid,
                            void* workspace, int reuse_x, const float* row_max, ntk_gemm_partials* defer, int full_form, hipStream_t st) {
    constexpr int PASS = ntk::GB_MAX_CHUNKS * ntk::GB_TOK;
    if (n_tokens > PASS) reuse_x = 0;   // the planes hold one pass (1024 tokens) at a time
    ntk::set_partials(defer, segs, nseg, n_tokens, 1, nullptr);   // (more than one pass: each pass reduces itself, nothing is deferred)
    if (n_tokens > PASS) defer = nullptr;
    for (int t0 = 0; t0 < n_tokens; t0 += PASS) {   // up to 16 x 64 tokens per launch: the chunks share the weights in L2
        const int T = std::min(PASS, n_tokens - t0);
        ntk::HostSeg sg[ntk::GB_MAX_SEG];
        for (int i = 0; i < nseg; ++i) sg[i] = ntk::HostSeg{segs[i].Y + (size_t)t0 * segs[i].out, segs[i].W, segs[i].out};
        const float* x = X + (size_t)t0 * in_features;
        const float* rs = resid ? resid + (size_t)t0 * segs[0].out : nullptr;
        const float* rm = row_max ? row_max + t0 : nullptr;
        const int rc = ntk::with_gemm_format(weight_dtype, [&](auto dt) {
            return ntk::launch_gemm_f16<decltype(dt)::value>(sg, nseg, x, T, in_features, rs, workspace, reuse_x, rm, defer, full_form != 0, st);
        });
        if (rc != NTK_OK) return rc;
    }
    return NTK_OK;
}

// The FP16 GEMM behind its descriptor (include/ntk_engine.h: ntk_gemm_desc): 1..3 matrices of one format sharing X, optional residual (one matrix),
// optional token maxima, optional deferral of the split-K sums to the consuming launch.
int ntk_gemm_quant_f16(const ntk_gemm_desc* d, void* stream) {
    if (!d || !d->segs || !d->X || !d->workspace) return NTK_E_NULL;
    const int nseg = d->nseg, n_tokens = d->n_tokens, in_features = d->in_features;
    if (nseg < 1 || nseg > ntk::GB_MAX_SEG || n_tokens < 0 || in_features <= 0 || (d->resid && nseg != 1)) return NTK_E_SHAPE;
    ntk::HostSeg sg[ntk::GB_MAX_SEG];
    long total = 0;
    for (int i = 0; i < nseg; ++i) {
        if (!d->segs[i].W || !d->segs[i].y) return NTK_E_NULL;
        if (d->segs[i].rows < 0 || (nseg > 1 && d->segs[i].rows == 0) || d->segs[i].dtype != d->segs[0].dtype) return NTK_E_SHAPE;
        sg[i] = ntk::HostSeg{d->segs[i].y, d->segs[i].W, d->segs[i].rows};
        total += d->segs[i].rows;
    }
    int dt = d->segs[0].dtype;
    if (dt != NTK_DT_Q8_0 && dt != NTK_DT_Q4_0 && dt != NTK_DT_Q4_K && dt != NTK_DT_Q5_K && dt != NTK_DT_Q6_K) return NTK_E_DTYPE;
    if (d->weights_repacked) {   // segs[i].W = tensors of the decode repack (ntk_rp_pack): the K-quant formats, rows in whole tiles of 16 (as everything here)
        if (dt != NTK_DT_Q4_K && dt != NTK_DT_Q5_K && dt != NTK_DT_Q6_K) return NTK_E_DTYPE;
        dt += ntk::GB_RP;
    }
    if (d->workspace_bytes < ntk_gemm_quant_workspace_bytes(in_features, (int)total) || (reinterpret_cast<uintptr_t>(d->workspace) & 15)) return NTK_E_SHAPE;
    ntk_gemm_partials* defer = d->partials;
    ntk::set_partials(defer, sg, nseg, n_tokens, 1, nullptr);
    if (n_tokens == 0 || total == 0) return NTK_OK;
    // (resid with partials: added by the launch's own epilogue when it does not split K -- nothing is deferred then; left to the consumer when it does)
    return gemm_ws_dispatch(sg, nseg, d->X, n_tokens, in_features, dt, d->resid, d->workspace, d->reuse_x, d->row_max, defer, d->full_form, ntk::resolve_stream(stream));
}

// hidden[t] += W . X[t] (the projection's splits summed here, residual last) and x_out[t] = rmsnorm(hidden[t]) with its largest |x|
int ntk_reduce_rmsnorm_rowmax(float* hidden, const ntk_gemm_partials* p, const float* weight, float eps, float* x_out, float* row_max,
                              float* zero_tokens, void* stream) {
    if (!hidden || !p || !weight || !x_out || !row_max) return NTK_E_NULL;
    if (p->nseg != 1 || p->n_tokens < 0 || p->rows[0] <= 0 || p->nsplit < 1) return NTK_E_SHAPE;
    if (p->n_tokens == 0) return NTK_OK;
    const int T = p->n_tokens, H = p->rows[0];
    hipStream_t st = ntk::resolve_stream(stream);
    const dim3 block(H <= 1024 ? 256 : (H <= 4096 ? 512 : 1024));
    if (p->nsplit == 1 || !p->part[0]) {   // the projection wrote Y itself: in place over hidden with the residual added by its epilogue (Y = resid = hidden), or
        if (p->y[0] != hidden) {              // Y = W . X elsewhere: hidden += Y first
            const size_t n4 = ((size_t)T * H + 3) / 4;
            if (((size_t)T * H) % 4 != 0 || (reinterpret_cast<uintptr_t>(hidden) & 15) || (reinterpret_cast<uintptr_t>(p->y[0]) & 15)) return NTK_E_ALIGN;
            ntk::ReduceArgs ra{};
            ra.nseg = 1; ra.T = T; ra.nsplit = 1; ra.resid = hidden; ra.Y[0] = hidden; ra.part[0] = p->y[0]; ra.out[0] = H;
            hipLaunchKernelGGL(ntk::reduce_splits_kernel, dim3((unsigned)((n4 + 255) / 256), 1), dim3(256), 0, st, ra);
        }
        hipLaunchKernelGGL(ntk::rmsnorm_rowmax_kernel, dim3(T), block, 0, st, x_out, hidden, weight, H, eps, row_max, zero_tokens);
        return ntk::last_launch_status();
    }
    hipLaunchKernelGGL(ntk::reduce_rmsnorm_rowmax_kernel, dim3(T), block, 0, st, hidden, p->part[0], p->nsplit, T, H, weight, eps, x_out, row_max, zero_tokens, static_cast<uint8_t*>(nullptr));
    return ntk::last_launch_status();
}
// out[t] = silu(gate[t]) * up[t] of a deferred gate | up launch (p: two matrices of equal height) with the tokens' largest |out|
int ntk_reduce_silu_mul_rowmax(float* output, const ntk_gemm_partials* p, float* row_max, void* stream) {
    if (!output || !p || !row_max) return NTK_E_NULL;
    if (p->nseg != 2 || p->rows[0] != p->rows[1] || p->rows[0] <= 0 || p->rows[0] % 4 != 0 || p->n_tokens < 0 || p->nsplit < 1) return NTK_E_SHAPE;
    if (p->n_tokens == 0) return NTK_OK;
    const int T = p->n_tokens, I = p->rows[0];
    if (T > 65535) return NTK_E_SHAPE;   // (tokens are gridDim.y; the engine's prompt pass never hands over more than 1024 at a time)
    if (p->nsplit == 1 || !p->part[0] || !p->part[1]) return ntk_silu_mul_rowmax(output, p->y[0], p->y[1], T, I, row_max, stream);
    if (reinterpret_cast<uintptr_t>(output) & 15) return NTK_E_ALIGN;
    hipLaunchKernelGGL(ntk::reduce_silu_mul_rowmax_kernel, dim3((I + 1023) / 1024, T), dim3(256), 0, ntk::resolve_stream(stream), output, p->part[0], p->part[1],
                       p->nsplit, T, I, row_max);
    return ntk::last_launch_status();
}

// ---- the operand pre-pass inside the producers (include/ntk_engine.h): planes, step sums and 1 / s of X[n_tokens][in] into `workspace`, for a projection that
// then runs with reuse_x = 1.  One pass (<= 1024 tokens); in a multiple of 32; every row 16-byte aligned.
static int prepare_x_check(const void* X, int n_tokens, int in, const void* workspace) {
    if (!X || !workspace) return NTK_E_NULL;
    if (n_tokens < 0 || in <= 0 || in % 32 != 0 || n_tokens > ntk::GB_MAX_CHUNKS * ntk::GB_TOK) return NTK_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(workspace)) & 15) return NTK_E_ALIGN;
    return NTK_OK;
}
int ntk_gemm_prepare_x(const float* X, int n_tokens, int in_features, void* workspace, void* stream) {
    const int st = prepare_x_check(X, n_tokens, in_features, workspace);
    if (st != NTK_OK || n_tokens == 0) return st;
    hipLaunchKernelGGL(ntk::rowmax_split_kernel, dim3(ntk::split_pad_tokens(n_tokens)), dim3(256), 0, ntk::resolve_stream(stream), X, n_tokens, in_features,
                       static_cast<uint8_t*>(workspace));
    return ntk::last_launch_status();
}
int ntk_rmsnorm_prepare_x(float* output, const float* input, const float* weight, int n_tokens, int hidden_size, float eps, void* workspace, void* stream) {
    if (!input || !weight) return NTK_E_NULL;
    const int st = prepare_x_check(output, n_tokens, hidden_size, workspace);
    if (st != NTK_OK || n_tokens == 0) return st;
    hipLaunchKernelGGL(ntk::rmsnorm_split_kernel, dim3(ntk::split_pad_tokens(n_tokens)), dim3(hidden_size <= 1024 ? 256 : (hidden_size <= 4096 ? 512 : 1024)) /* = ntk_rmsnorm's blocks */,
                       0, ntk::resolve_stream(stream), output, input, weight, n_tokens, hidden_size, eps, static_cast<uint8_t*>(workspace));
    return ntk::last_launch_status();
}
// ntk_reduce_rmsnorm_rowmax with the split instead of the row maxima (same sums, same normalisation: x_out holds the same bits)
int ntk_reduce_rmsnorm_prepare_x(float* hidden, const ntk_gemm_partials* p, const float* weight, float eps, float* x_out, void* workspace, void* stream) {
    if (!hidden || !p || !weight) return NTK_E_NULL;
    if (p->nseg != 1 || p->n_tokens < 0 || p->rows[0] <= 0 || p->nsplit < 1) return NTK_E_SHAPE;
    const int T = p->n_tokens, H = p->rows[0];
    const int st0 = prepare_x_check(x_out, T, H, workspace);
    if (st0 != NTK_OK || T == 0) return st0;
    hipStream_t st = ntk::resolve_stream(stream);
    const dim3 block(H <= 1024 ? 256 : (H <= 4096 ? 512 : 1024));
    if (p->nsplit == 1 || !p->part[0]) {   // (as ntk_reduce_rmsnorm_rowmax: the projection wrote Y itself)
        if (p->y[0] != hidden) {
            const size_t n4 = ((size_t)T * H + 3) / 4;
            if (((size_t)T * H) % 4 != 0 || (reinterpret_cast<uintptr_t>(hidden) & 15) || (reinterpret_cast<uintptr_t>(p->y[0]) & 15)) return NTK_E_ALIGN;
            ntk::ReduceArgs ra{};
            ra.nseg = 1; ra.T = T; ra.nsplit = 1; ra.resid = hidden; ra.Y[0] = hidden; ra.part[0] = p->y[0]; ra.out[0] = H;
            hipLaunchKernelGGL(ntk::reduce_splits_kernel, dim3((unsigned)((n4 + 255) / 256), 1), dim3(256), 0, st, ra);
        }
        hipLaunchKernelGGL(ntk::rmsnorm_split_kernel, dim3(ntk::split_pad_tokens(T)), block, 0, st, x_out, hidden, weight, T, H, eps, static_cast<uint8_t*>(workspace));
        return ntk::last_launch_status();
    }
    hipLaunchKernelGGL(ntk::reduce_rmsnorm_rowmax_kernel, dim3(ntk::split_pad_tokens(T)), block, 0, st, hidden, p->part[0], p->nsplit, T, H, weight, eps, x_out,
                       static_cast<float*>(nullptr), static_cast<float*>(nullptr), static_cast<uint8_t*>(workspace));
    return ntk::last_launch_status();
}
int ntk_silu_mul_prepare_x(float* output, const float* gate, const float* up, int n_tokens, int width, void* workspace, void* stream) {
    if (!gate || !up) return NTK_E_NULL;
    const int st = prepare_x_check(output, n_tokens, width, workspace);
    if (st != NTK_OK || n_tokens == 0) return st;
    if ((reinterpret_cast<uintptr_t>(gate) | reinterpret_cast<uintptr_t>(up)) & 15) return NTK_E_ALIGN;
    hipLaunchKernelGGL(ntk::silu_mul_split_kernel, dim3(ntk::split_pad_tokens(n_tokens)), dim3(1024), 0, ntk::resolve_stream(stream), output, gate, up, 1, n_tokens, width,
                       static_cast<uint8_t*>(workspace));
    return ntk::last_launch_status();
}
// (`workspace` must not be the workspace the partial sums lie in: the launch reads those while it writes the planes)
int ntk_reduce_silu_mul_prepare_x(float* output, const ntk_gemm_partials* p, void* workspace, void* stream) {
    if (!p) return NTK_E_NULL;
    if (p->nseg != 2 || p->rows[0] != p->rows[1] || p->rows[0] <= 0 || p->n_tokens < 0 || p->nsplit < 1) return NTK_E_SHAPE;
    const int T = p->n_tokens, I = p->rows[0];
    if (p->nsplit == 1 || !p->part[0] || !p->part[1]) return ntk_silu_mul_prepare_x(output, p->y[0], p->y[1], T, I, workspace, stream);
    const int st = prepare_x_check(output, T, I, workspace);
    if (st != NTK_OK || T == 0) return st;
    hipLaunchKernelGGL(ntk::silu_mul_split_kernel, dim3(ntk::split_pad_tokens(T)), dim3(1024), 0, ntk::resolve_stream(stream), output, p->part[0], p->part[1], p->nsplit, T, I,
                       static_cast<uint8_t*>(workspace));
    return ntk::last_launch_status();
}

int ntk_rmsnorm_rowmax(float* output, const float* input, const float* weight, int n_tokens, int hidden_size, float eps, float* row_max,
                       float* zero_tokens, void* stream) {
    if (!output || !input || !weight || !row_max) return NTK_E_NULL;
    if (n_tokens < 0 || hidden_size <= 0) return NTK_E_SHAPE;
    if (n_tokens == 0) return NTK_OK;
    hipLaunchKernelGGL(ntk::rmsnorm_rowmax_kernel, dim3(n_tokens), dim3(hidden_size <= 1024 ? 256 : (hidden_size <= 4096 ? 512 : 1024)) /* = ntk_rmsnorm's blocks: the same sums */, 0,
                       ntk::resolve_stream(stream), output, input,
                       weight, hidden_size, eps, row_max, zero_tokens);
    return ntk::last_launch_status();
}
int ntk_silu_mul_rowmax(float* output, const float* gate, const float* up, int n_tokens, int width, float* row_max, void* stream) {
    if (!output || !gate || !up || !row_max) return NTK_E_NULL;
    if (n_tokens < 0 || width <= 0 || width % 4 != 0) return NTK_E_SHAPE;
    if (n_tokens > 65535) return NTK_E_SHAPE;   // tokens are gridDim.y: the caller falls back to ntk_silu_mul (model.cpp) / splits the prompt
    if ((reinterpret_cast<uintptr_t>(output) | reinterpret_cast<uintptr_t>(gate) | reinterpret_cast<uintptr_t>(up)) & 15) return NTK_E_ALIGN;
    if (n_tokens == 0) return NTK_OK;
    hipLaunchKernelGGL(ntk::silu_mul_rowmax_kernel, dim3((width + 1023) / 1024, n_tokens), dim3(256), 0, ntk::resolve_stream(stream), output, gate, up, width,
                       row_max);
    return ntk::last_launch_status();
}

}  // extern "C"
