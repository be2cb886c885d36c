// moe_core.hip.h -- the device functions the two forms of the routed expert FFN share: the T-row launches of moe.hip and the one-row form of moe_row.hip.
// Everything that decides a BIT of the result lives here once -- the router's dot, the selection and its softmax, the staging of a GGUF row into a wave's LDS
// image, the decode of a 32-column unit and the one FMA chain over a lane's units -- so the two forms cannot drift apart.
#pragma once
#include "common.hip.h"

namespace ntk {

typedef uint32_t moe_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMoeMaxE = 256, kMoeMaxK = 16, kMoeMaxT = 1024;

__host__ __device__ inline bool moe_type_ok(int dt) { return dt == NTK_DT_Q8_0 || dt == NTK_DT_Q4_K || dt == NTK_DT_Q6_K; }
// bytes of one row's LDS image: the row behind a shift of up to 14 bytes, whole 16-byte pieces, and the dword the unaligned reads may touch behind it
__host__ __device__ inline unsigned moe_image_bytes(unsigned row_bytes) { return (row_bytes + 15u + 15u) / 16u * 16u + 16u; }

// ---- a row's bytes into the wave's image: st[shift + k] = g[k], shift = the row address's low four bits (so aligned pieces stay aligned) ----
__device__ __forceinline__ int moe_stage_row(uint8_t* st, const uint8_t* g, unsigned rb, int lane) {
    const unsigned shift = (unsigned)((uintptr_t)g & 15u);
    unsigned head = (16u - shift) & 15u;
    if (head > rb) head = rb;
    const unsigned body = (rb - head) / 16u, tail = rb - head - 16u * body;
    for (unsigned i = lane; i < head / 2u; i += 64u) reinterpret_cast<uint16_t*>(st + shift)[i] = reinterpret_cast<const uint16_t*>(g)[i];
    const moe_u32x4* src = reinterpret_cast<const moe_u32x4*>(g + head);
    moe_u32x4* dst = reinterpret_cast<moe_u32x4*>(st + shift + head);
    for (unsigned i = lane; i < body; i += 64u) dst[i] = src[i];
    const unsigned t0 = head + 16u * body;
    for (unsigned i = lane; i < tail / 2u; i += 64u) reinterpret_cast<uint16_t*>(st + shift + t0)[i] = reinterpret_cast<const uint16_t*>(g + t0)[i];
    return (int)shift;
}

// ---- the 32 weights of unit u of a staged row (o: the image offset of the row's first byte), as floats in column order ----
template <int DT> __device__ __forceinline__ void moe_decode_unit(float (&w)[32], const uint8_t* st, int o, int u);

template <> __device__ __forceinline__ void moe_decode_unit<NTK_DT_Q8_0>(float (&w)[32], const uint8_t* st, int o, int u) {
    const int ob = o + 34 * u;
    const float d = h2f(lds_u16_at(st, ob));
    uint32_t q[8];
    lds_read_dwords<8>(q, st, ob + 2);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) w[4 * i + k] = d * sb2f(q[i], k);
}

template <> __device__ __forceinline__ void moe_decode_unit<NTK_DT_Q4_K>(float (&w)[32], const uint8_t* st, int o, int u) {
    const int j = u & 7, ob = o + 144 * (u >> 3);   // sub-block j of the block: columns 32 j .., the low (j even) or high nibbles of qs[32 (j / 2) ..]
    uint32_t hd[4], q[8];
    lds_read_dwords<4>(hd, st, ob);
    const float d = h2f((uint16_t)(hd[0] & 0xFFFFu)), dmin = h2f((uint16_t)(hd[0] >> 16));
    float sc, mn;
    kq_scale_min(hd[1], hd[2], hd[3], j, sc, mn);
    lds_read_dwords<8>(q, st, ob + 16 + 32 * (j >> 1));
    const float ds = d * sc, dm = dmin * mn;
    const int sh = 4 * (j & 1);
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) w[4 * i + k] = ds * (float)((q[i] >> (8 * k + sh)) & 15u) - dm;
}

template <> __device__ __forceinline__ void moe_decode_unit<NTK_DT_Q6_K>(float (&w)[32], const uint8_t* st, int o, int u) {
    // unit r of the block: half hf = r / 4, type t = r % 4 -- columns 128 hf + 32 t ..: ql[64 hf + 32 (t & 1) + l] (low nibble for t < 2, else high),
    // the two top bits at bits 2 t of qh[32 hf + l], sub-scale 8 hf + 2 t + l / 16
    const int r = u & 7, hf = r >> 2, t = r & 3, ob = o + 210 * (u >> 3);
    uint32_t ql[8], qh[8];
    lds_read_dwords<8>(ql, st, ob + 64 * hf + 32 * (t & 1));
    lds_read_dwords<8>(qh, st, ob + 128 + 32 * hf);
    const uint32_t scb = lds_u16_at(st, ob + 192 + 8 * hf + 2 * t);
    const float d = h2f(lds_u16_at(st, ob + 208));
    const float s0 = d * sb2f(scb, 0), s1 = d * sb2f(scb, 1);
    const int nsh = 4 * (t >> 1), hsh = 2 * t;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t lo = (ql[i] >> (8 * k + nsh)) & 15u, hi = (qh[i] >> (8 * k + hsh)) & 3u;
            w[4 * i + k] = (i < 4 ? s0 : s1) * (float)((int)(lo | (hi << 4)) - 32);
        }
}

// acc[j] += sum over the lane's units of w . x_j: one FMA chain per pair, columns ascending
template <int DT, int NP>
__device__ __forceinline__ void moe_units(float (&acc)[NP], const uint8_t* st, int o, int n_units, int lane, const float* const (&x)[NP]) {
    for (int u = lane; u < n_units; u += 64) {
        float w[32];
        moe_decode_unit<DT>(w, st, o, u);
#pragma unroll
        for (int j = 0; j < NP; ++j) {
            const float4* xp = reinterpret_cast<const float4*>(x[j] + 32 * u);
            float a = acc[j];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float4 v = xp[i];
                a = fmaf(w[4 * i], v.x, a);
                a = fmaf(w[4 * i + 1], v.y, a);
                a = fmaf(w[4 * i + 2], v.z, a);
                a = fmaf(w[4 * i + 3], v.w, a);
            }
            acc[j] = a;
        }
    }
}
// NP = the pairs of one pass over a staged row, or 1 for a lone pair (a decode token: every active expert has one): the same chain per pair, so the same
// bits, without the discarded copies
template <int NP>
__device__ __forceinline__ void moe_row_dots(float (&acc)[NP], int dt, const uint8_t* st, int o, int n_units, int lane, const float* const (&x)[NP]) {
#pragma unroll
    for (int j = 0; j < NP; ++j) acc[j] = 0.0f;
    if (dt == NTK_DT_Q8_0) moe_units<NTK_DT_Q8_0, NP>(acc, st, o, n_units, lane, x);
    else if (dt == NTK_DT_Q4_K) moe_units<NTK_DT_Q4_K, NP>(acc, st, o, n_units, lane, x);
    else moe_units<NTK_DT_Q6_K, NP>(acc, st, o, n_units, lane, x);
#pragma unroll
    for (int j = 0; j < NP; ++j) acc[j] = wave_sum(acc[j]);
}

// ---- the router's logit of one expert, by one wave: lane l takes the float4 pieces l, l + 64, ... (vec), or the elements l, l + 64, ... ----
__device__ __forceinline__ float moe_router_dot(const float* x, const float* r, int hidden, int vec, int lane) {
    float s = 0.0f;
    if (vec) {
        for (int i = lane; i < hidden / 4; i += 64) {
            const float4 xv = reinterpret_cast<const float4*>(x)[i], rv = reinterpret_cast<const float4*>(r)[i];
            s = fmaf(rv.x, xv.x, s); s = fmaf(rv.y, xv.y, s); s = fmaf(rv.z, xv.z, s); s = fmaf(rv.w, xv.w, s);
        }
    } else {
        for (int i = lane; i < hidden; i += 64) s = fmaf(r[i], x[i], s);
    }
    return wave_sum(s);
}

// ---- the K largest of E logits, by one wave: lane l holds experts l, l + 64, l + 128, l + 192; K rounds of (largest value, lowest index) over the entries
//      not yet taken.  Every lane ends with all K (sel, sel_id), in descending order. ----
__device__ __forceinline__ void moe_select(const float* logit, int E, int K, int lane, float (&sel)[kMoeMaxK], int (&sel_id)[kMoeMaxK]) {
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = lane + 64 * j;
        const float f = e < E ? logit[e] : -INFINITY;
        v[j] = f == f ? f : -INFINITY;   // (a NaN logit ranks last instead of poisoning the comparisons)
    }
    unsigned taken = 0;
#pragma unroll
    for (int k = 0; k < kMoeMaxK; ++k) { sel[k] = 0.0f; sel_id[k] = 0; }
    for (int k = 0; k < K; ++k) {
        float bv = -INFINITY;
        int bi = 0x7FFFFFFF;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = lane + 64 * j;
            if (e < E && !((taken >> j) & 1u) && (bi == 0x7FFFFFFF || v[j] > bv)) { bv = v[j]; bi = e; }
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const float ov = __shfl_xor(bv, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (oi != 0x7FFFFFFF && (bi == 0x7FFFFFFF || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
        }
        if ((bi & 63) == lane) taken |= 1u << (bi >> 6);
#pragma unroll
        for (int kk = 0; kk < kMoeMaxK; ++kk) if (kk == k) { sel[kk] = bv; sel_id[kk] = bi; }
    }
}

// ---- one thread: softmax over the K selected logits (the largest comes first), ids[k] and w[k] = ex[k] / sum stored ----
__device__ __forceinline__ void moe_softmax_store(const float (&sel)[kMoeMaxK], const int (&sel_id)[kMoeMaxK], int K, int* ids, float* w) {
    float ex[kMoeMaxK], sum = 0.0f;
#pragma unroll
    for (int k = 0; k < kMoeMaxK; ++k) {
        ex[k] = k < K ? expf(sel[k] - sel[0]) : 0.0f;
        if (k < K) sum += ex[k];
    }
#pragma unroll
    for (int k = 0; k < kMoeMaxK; ++k)
        if (k < K) {
            ids[k] = sel_id[k];
            w[k] = ex[k] / sum;
        }
}

// SiLU(g) x u, as every form of the gate | up product ends
__device__ __forceinline__ float moe_silu_mul(float g, float u) { return g / (1.0f + expf(-g)) * u; }

}  // namespace ntk
