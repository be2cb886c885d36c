// gemm_deq.hip.h -- raw GGUF blocks as F32 A-operands of v_mfma_f32_16x16x4_f32: the block geometry (GFmt) and the per-lane decoders (Deq) that the
// matrix-core GEMMs over quantised weights share -- the dense prompt GEMM (gemm_prefill.hip) and the grouped expert GEMM (moe_gemm.hip).  A decoder reads
// an LDS image of a row's bytes and returns the 8 weights of one (32-column sub-block, column group) in column order, dequantised exactly as the GEMV
// kernels define them (reference gemm.cu:60-75, 129-141, 190-244, 297-354, 421-459 / SURVEY.md Appendix A).
#pragma once
#include "common.hip.h"

namespace ntk {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int DT> struct GFmt;
// BW/BB: weights / bytes per block.  PIECES: 16-byte pieces that cover one row's slice bytes at any 2-byte alignment.
template <> struct GFmt<NTK_DT_Q8_0> { static constexpr int BW = 32, BB = 34, SB = 272; };
template <> struct GFmt<NTK_DT_Q4_0> { static constexpr int BW = 32, BB = 18, SB = 144; };
template <> struct GFmt<NTK_DT_Q4_K> { static constexpr int BW = 256, BB = 144, SB = 144; };
template <> struct GFmt<NTK_DT_Q5_K> { static constexpr int BW = 256, BB = 176, SB = 176; };
template <> struct GFmt<NTK_DT_Q6_K> { static constexpr int BW = 256, BB = 210, SB = 210; };
// Unquantised 16-bit rows (IEEE half, bfloat16): a "block" is 32 consecutive weights in 64 bytes, no scale.  A chunk of a row is then 8 KiB, and
// sixteen of them with the padded pitch would not fit the CU's 160 KiB beside the reduction buffers; these formats require 16-byte-aligned rows
// instead (W aligned; a row is a multiple of 64 bytes), stage exactly 8 KiB per row at a pitch of 8 KiB and keep the reads conflict-free by
// XOR-ing the 16-byte piece index with the row (SWZ: kernel stage + Deq16 below) -- 160 KiB to the byte.
template <> struct GFmt<NTK_DT_F16>  { static constexpr int BW = 32, BB = 64, SB = 512; };
template <> struct GFmt<NTK_DT_BF16> { static constexpr int BW = 32, BB = 64, SB = 512; };
template <int DT> constexpr bool GSWZ = (DT == NTK_DT_F16 || DT == NTK_DT_BF16);

// The 8 weights of (row image `st`, 32-column sub-block s of the slice, column group g) as F32.
//   st: LDS image of the row's slice bytes, byte k of the slice at st[k] (st itself carries the row's alignment shift)
template <int DT> struct Deq;

__device__ __forceinline__ void bytes8_to_f32(uint32_t lo, uint32_t hi, float (&f)[8]) {
    f[0] = ub2f(lo, 0); f[1] = ub2f(lo, 1); f[2] = ub2f(lo, 2); f[3] = ub2f(lo, 3);
    f[4] = ub2f(hi, 0); f[5] = ub2f(hi, 1); f[6] = ub2f(hi, 2); f[7] = ub2f(hi, 3);
}

template <> struct Deq<NTK_DT_Q8_0> {   // gemm.cu:129-141: w = d * q
    __device__ static void run(const uint8_t* st, int shift, int s, int g, float (&a)[8]) {
        const int ob = shift + 34 * s;
        const float d = h2f(lds_u16_at(st, ob));
        uint32_t q[2];
        lds_read_dwords<2>(q, st, ob + 2 + 8 * g);
#pragma unroll
        for (int j = 0; j < 4; ++j) { a[j] = d * sb2f(q[0], j); a[4 + j] = d * sb2f(q[1], j); }
    }
};

template <> struct Deq<NTK_DT_Q4_0> {   // gemm.cu:60-75: columns 0..15 low nibbles, 16..31 high nibbles; w = d (n - 8)
    __device__ static void run(const uint8_t* st, int shift, int s, int g, float (&a)[8]) {
        const int ob = shift + 18 * s;
        const float d = h2f(lds_u16_at(st, ob));
        uint32_t q[2];
        lds_read_dwords<2>(q, st, ob + 2 + 8 * (g & 1));
        const int sh = 4 * (g >> 1);
        float n[8];
        bytes8_to_f32((q[0] >> sh) & 0x0F0F0F0Fu, (q[1] >> sh) & 0x0F0F0F0Fu, n);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = d * (n[j] - 8.0f);
    }
};

// K-quant (scale, min) of sub-block s (types.h:112-117, gemm.cu:206-222); hd = the block's first 16 bytes
__device__ __forceinline__ void kq_pair(const uint32_t (&hd)[4], int s, float& dsc, float& dmn) {
    const float d = h2f((uint16_t)(hd[0] & 0xFFFFu)), dmin = h2f((uint16_t)(hd[0] >> 16));
    const uint32_t s0 = hd[1], s1 = hd[2], s2 = hd[3];
    uint32_t sc, mn;
    if (s < 4) {
        sc = (s0 >> (8 * s)) & 63u;
        mn = (s1 >> (8 * s)) & 63u;
    } else {
        const int b = 8 * (s - 4);
        sc = ((s2 >> b) & 0xFu) | (((s0 >> (b + 6)) & 3u) << 4);
        mn = ((s2 >> (b + 4)) & 0xFu) | (((s1 >> (b + 6)) & 3u) << 4);
    }
    dsc = d * (float)sc;
    dmn = dmin * (float)mn;
}

template <> struct Deq<NTK_DT_Q4_K> {   // gemm.cu:190-244: w = d sc n - dmin m
    __device__ static void run(const uint8_t* st, int shift, int s, int g, float (&a)[8]) {
        uint32_t hd[4], q[2];
        lds_read_dwords<4>(hd, st, shift);
        float dsc, dmn;
        kq_pair(hd, s, dsc, dmn);
        lds_read_dwords<2>(q, st, shift + 16 + 32 * (s >> 1) + 8 * g);
        const int sh = 4 * (s & 1);
        float n[8];
        bytes8_to_f32((q[0] >> sh) & 0x0F0F0F0Fu, (q[1] >> sh) & 0x0F0F0F0Fu, n);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = fmaf(dsc, n[j], -dmn);
    }
};

template <> struct Deq<NTK_DT_Q5_K> {   // gemm.cu:297-354: fifth bit = bit s of qh[l]
    __device__ static void run(const uint8_t* st, int shift, int s, int g, float (&a)[8]) {
        uint32_t hd[4], q[2], h[2];
        lds_read_dwords<4>(hd, st, shift);
        float dsc, dmn;
        kq_pair(hd, s, dsc, dmn);
        lds_read_dwords<2>(h, st, shift + 16 + 8 * g);
        lds_read_dwords<2>(q, st, shift + 48 + 32 * (s >> 1) + 8 * g);
        const int sh = 4 * (s & 1);
        float n[8];
        bytes8_to_f32(((q[0] >> sh) & 0x0F0F0F0Fu) | (((h[0] >> s) & 0x01010101u) << 4),
                      ((q[1] >> sh) & 0x0F0F0F0Fu) | (((h[1] >> s) & 0x01010101u) << 4), n);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = fmaf(dsc, n[j], -dmn);
    }
};

template <> struct Deq<NTK_DT_Q6_K> {   // gemm.cu:421-459: sub-block s = 4 half + type; w = d sc[8 half + 2 type + l/16] (q - 32)
    __device__ static void run(const uint8_t* st, int shift, int s, int g, float (&a)[8]) {
        const int hf = s >> 2, ty = s & 3;
        uint32_t q[2], h[2];
        lds_read_dwords<2>(q, st, shift + 64 * hf + 32 * (ty & 1) + 8 * g);
        lds_read_dwords<2>(h, st, shift + 128 + 32 * hf + 8 * g);
        const uint32_t scw = (uint32_t)lds_u16_at(st, shift + 192 + 8 * hf + 2 * ty);   // the sub-block's two int8 sub-scales
        const float d = h2f(lds_u16_at(st, shift + 208));
        const float dsc = d * sb2f(scw, 0) , dsc1 = d * sb2f(scw, 1);
        const float sc = (g >> 1) ? dsc1 : dsc;                                          // l / 16 = g / 2
        const int sh = 4 * (ty >> 1);
        float n[8];
        bytes8_to_f32(((q[0] >> sh) & 0x0F0F0F0Fu) | (((h[0] >> (2 * ty)) & 0x03030303u) << 4),
                      ((q[1] >> sh) & 0x0F0F0F0Fu) | (((h[1] >> (2 * ty)) & 0x03030303u) << 4), n);
#pragma unroll
        for (int j = 0; j < 8; ++j) a[j] = sc * (n[j] - 32.0f);
    }
};

// 16-bit rows: the lane's 8 weights are ONE 16-byte piece of the swizzled row image (piece index ^ row, row = lane % 16 -- the kernel's r), widened
// exactly: half by v_cvt_f32_f16, bfloat16 as the high half of the float
template <bool BF> struct Deq16 {
    __device__ static void run(const uint8_t* st, int shift, int s, int g, float (&a)[8]) {
        const int piece = ((shift + 64 * s + 16 * g) >> 4) ^ ((int)threadIdx.x & 15);
        const u32x4 v = *reinterpret_cast<const u32x4*>(st + 16 * piece);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if constexpr (BF) { a[2 * j] = __uint_as_float(w[j] << 16); a[2 * j + 1] = __uint_as_float(w[j] & 0xFFFF0000u); }
            else { a[2 * j] = h2f((uint16_t)(w[j] & 0xFFFFu)); a[2 * j + 1] = h2f((uint16_t)(w[j] >> 16)); }
        }
    }
};
template <> struct Deq<NTK_DT_F16> : Deq16<false> {};
template <> struct Deq<NTK_DT_BF16> : Deq16<true> {};

}  // namespace ntk
