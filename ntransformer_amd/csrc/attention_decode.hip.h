// attention_decode.hip.h -- the device functions of the decode attention kernels (attention.hip), shared with the batched form
// (attention_batch.hip): the helpers, the three-pass `attend` core with the generic fused row around it, the single-pass / split-KV walk and
// the merge of the split states.  A kernel is a thin __global__ wrapper that says which (row, head, split) a workgroup serves.
#pragma once
#include "common.hip.h"
#include "attention_merge.hip.h"
#include <cfloat>
#include <cstdlib>

namespace ntk {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ void unpack8(const u32x4 r, float (&f)[8]) {
    f[0] = h2f((uint16_t)(r.x & 0xFFFF)); f[1] = h2f((uint16_t)(r.x >> 16));
    f[2] = h2f((uint16_t)(r.y & 0xFFFF)); f[3] = h2f((uint16_t)(r.y >> 16));
    f[4] = h2f((uint16_t)(r.z & 0xFFFF)); f[5] = h2f((uint16_t)(r.z >> 16));
    f[6] = h2f((uint16_t)(r.w & 0xFFFF)); f[7] = h2f((uint16_t)(r.w >> 16));
}

// acc[0..7] += (the eight halves of r) * p, one v_fma_mix_f32 each: the instruction converts its F16 operand on the fly (exactly: the same
// bits as v_cvt_f32_f16 + v_fma_f32).  hipcc folds the conversion of the K rows into it by itself but turns the P.V update into v_cvt +
// v_pk_fma_f32 -- 1.5 issue slots per product (a packed FMA costs two, tools/probes/mfma_valu_probe.hip) against 1 here.  One asm block
// per position, behind an s_nop: p comes straight out of v_exp_f32, and a VALU instruction that reads a transcendental's result needs a
// wait state the compiler supplies for its own instructions but cannot supply inside opaque asm (without it the first product of every
// position read the PREVIOUS p in the lanes the quarter-rate v_exp had not written yet: found by the parity tests).
#ifdef NTK_ATTN_NO_ASM
__device__ __forceinline__ void pv_update(float (&acc)[8], const u32x4 r, const float p) {
    const uint32_t w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        acc[2 * i] = fmaf(p, h2f((uint16_t)(w[i] & 0xFFFFu)), acc[2 * i]);
        acc[2 * i + 1] = fmaf(p, h2f((uint16_t)(w[i] >> 16)), acc[2 * i + 1]);
    }
}
#else
__device__ __forceinline__ void pv_update(float (&acc)[8], const u32x4 r, const float p) {
    asm("s_nop 1\n\t"
        "v_fma_mix_f32 %0, %8, %12, %0 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %1, %8, %12, %1 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %2, %9, %12, %2 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %3, %9, %12, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %4, %10, %12, %4 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %5, %10, %12, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %6, %11, %12, %6 op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %7, %11, %12, %7 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "+v"(acc[0]), "+v"(acc[1]), "+v"(acc[2]), "+v"(acc[3]), "+v"(acc[4]), "+v"(acc[5]), "+v"(acc[6]), "+v"(acc[7])
        : "v"(r.x), "v"(r.y), "v"(r.z), "v"(r.w), "v"(p));
}
#endif

// rotation of one (x0, x1) pair, reference rotary.cu:46-60 (the frequency: rope_freq, common.hip.h)
__device__ __forceinline__ void rope_pair(float& x0, float& x1, int pos, int pair_idx, int head_dim, float theta, float fscale,
                                          const float* __restrict__ inv_freq = nullptr) {
    const float freq = rope_freq(inv_freq, pair_idx, head_dim, theta);
    const float angle = pos * freq * fscale;
    const float c = cosf(angle), s = sinf(angle);
    const float a = x0, b = x1;
    rope_rotate(a, b, c, s, x0, x1);
}

// ---------------------------------------------------------------------------------------------
// Core: softmax(q . K^T * scale) . V for ONE (head, query) pair, executed by one workgroup.
//   qs      : LDS, post-RoPE query [hd]
//   n_cache : keys/values 0..n_cache-1 are read from the cache
//   extra   : optional one more (key, value) pair held in LDS as floats (the token being decoded)
//   sc      : LDS scores [n_cache + 1]; part: LDS [nwaves][hd]; red: LDS [16]
// LPR = lanes per cache row (head_dim / 8); 0 selects the generic any-head_dim path.
// ---------------------------------------------------------------------------------------------
template <int LPR>
__device__ void attend(float* out, const float* qs, const uint16_t* kc, const uint16_t* vc, int n_cache,
                       const float* k_extra, const float* v_extra, int kv_head, int n_kv_heads, int hd,
                       float scale, float* sc, float* part, float* red) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, nwaves = blockDim.x >> 6;
    const size_t stride = (size_t)n_kv_heads * hd;
    const uint16_t* kbase = kc + (size_t)kv_head * hd;
    const uint16_t* vbase = vc + (size_t)kv_head * hd;
    const int n_keys = n_cache + (k_extra ? 1 : 0);

    // ---- phase 1: scores ------------------------------------------------------------------------
    if constexpr (LPR > 0) {
        constexpr int PPW = 64 / LPR;               // positions per wave instruction
        const int sub = lane / LPR, part_i = lane % LPR;
        float qreg[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) qreg[j] = qs[8 * part_i + j];
        for (int p0 = wave * PPW; p0 < n_cache; p0 += nwaves * PPW) {
            const int pos = p0 + sub;
            float s = 0.0f;
            if (pos < n_cache) {
                const u32x4 raw = *reinterpret_cast<const u32x4*>(kbase + pos * stride + 8 * part_i);
                float kf[8];
                unpack8(raw, kf);
#pragma unroll
                for (int j = 0; j < 8; ++j) s = fmaf(qreg[j], kf[j], s);
            }
            s = group_sum<LPR>(s);
            if (part_i == 0 && pos < n_cache) sc[pos] = s * scale;
        }
    } else {
        for (int pos = tid; pos < n_cache; pos += blockDim.x) {
            const uint16_t* k = kbase + pos * stride;
            float s = 0.0f;
            for (int d = 0; d < hd; ++d) s = fmaf(qs[d], h2f(k[d]), s);
            sc[pos] = s * scale;
        }
    }
    if (k_extra && wave == 0) {
        float s = 0.0f;
        for (int d = lane; d < hd; d += 64) s = fmaf(qs[d], k_extra[d], s);
        s = wave_sum(s);
        if (lane == 0) sc[n_cache] = s * scale;
    }
    __syncthreads();

    // ---- phase 2: softmax over sc[0..n_keys) -----------------------------------------------------
    float m = -FLT_MAX;
    for (int pos = tid; pos < n_keys; pos += blockDim.x) m = fmaxf(m, sc[pos]);
    m = block_max(m, red);
    float l = 0.0f;
    for (int pos = tid; pos < n_keys; pos += blockDim.x) {
        const float e = expf(sc[pos] - m);
        sc[pos] = e;
        l += e;
    }
    l = block_sum(l, red);
    const float inv = (l > 0.0f) ? 1.0f / l : 0.0f;   // reference attention.cu:293 (prefill guard); decode never hits 0
    __syncthreads();

    // ---- phase 3: out[d] = inv * sum_pos e[pos] V[pos][d] ------------------------------------------
    if constexpr (LPR > 0) {
        constexpr int PPW = 64 / LPR;
        const int sub = lane / LPR, part_i = lane % LPR;
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
        for (int p0 = wave * PPW; p0 < n_cache; p0 += nwaves * PPW) {
            const int pos = p0 + sub;
            if (pos < n_cache) {
                const float pw = sc[pos];
                const u32x4 raw = *reinterpret_cast<const u32x4*>(vbase + pos * stride + 8 * part_i);
                float vf[8];
                unpack8(raw, vf);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[j] = fmaf(pw, vf[j], acc[j]);
            }
        }
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] += __shfl_xor(acc[j], off, 64);
        }
        if (sub == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) part[wave * hd + 8 * part_i + j] = acc[j];
        }
        __syncthreads();
        for (int d = tid; d < hd; d += blockDim.x) {
            float t = 0.0f;
            for (int w = 0; w < nwaves; ++w) t += part[w * hd + d];
            if (v_extra) t = fmaf(sc[n_cache], v_extra[d], t);
            out[d] = t * inv;
        }
    } else {
        for (int d = tid; d < hd; d += blockDim.x) {
            float t = 0.0f;
            for (int pos = 0; pos < n_cache; ++pos) t = fmaf(sc[pos], h2f(vbase[pos * stride + d]), t);
            if (v_extra) t = fmaf(sc[n_cache], v_extra[d], t);
            out[d] = t * inv;
        }
    }
}

// RoPE + KV store + `attend` for one query head of one row (any head_dim): the body of attention_decode_fused_kernel
template <int LPR>
__device__ __forceinline__ void attention_decode_fused_row(
    float* __restrict__ output, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, const int* __restrict__ d_pos, int n_heads, int n_kv_heads,
    int hd, int max_seq, float scale, float theta, float fscale, const int head) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int group = n_heads / n_kv_heads, kv_head = head / group;
    const int pos = *d_pos;
    float* qs = lds;                        // [hd] post-RoPE query
    float* kx = qs + hd;                    // [hd] post-RoPE key of this token, rounded through half
    float* vx = kx + hd;                    // [hd] value of this token, rounded through half
    float* red = vx + hd;
    float* part = red + 16;
    float* sc = part + (blockDim.x >> 6) * hd;
    const int half_dim = hd / 2;
    const size_t cache_row = ((size_t)pos * n_kv_heads + kv_head) * hd;
    const bool writer = (head % group == 0) && pos < max_seq;   // one workgroup per kv head stores the row
    for (int i = threadIdx.x; i < half_dim; i += blockDim.x) {
        float a = q[(size_t)head * hd + i], b = q[(size_t)head * hd + i + half_dim];
        rope_pair(a, b, pos, i, hd, theta, fscale);
        qs[i] = a; qs[i + half_dim] = b;
        float ka = k[(size_t)kv_head * hd + i], kb = k[(size_t)kv_head * hd + i + half_dim];
        rope_pair(ka, kb, pos, i, hd, theta, fscale);
        const uint16_t ha = f2h(ka), hb = f2h(kb);          // reference attention.cu:338 (__float2half, RNE)
        kx[i] = h2f(ha); kx[i + half_dim] = h2f(hb);
        if (writer) { kc[cache_row + i] = ha; kc[cache_row + i + half_dim] = hb; }
    }
    for (int i = threadIdx.x; i < hd; i += blockDim.x) {
        const uint16_t hv = f2h(v[(size_t)kv_head * hd + i]);
        vx[i] = h2f(hv);
        if (writer) vc[cache_row + i] = hv;
    }
    __syncthreads();
    attend<LPR>(output + (size_t)head * hd, qs, kc, vc, pos, kx, vx, kv_head, n_kv_heads, hd, scale, sc, part, red);
}

// ---------------------------------------------------------------------------------------------
// Decode attention, single pass (engine path).  The reference kernel (attention.cu:108-202) and `attend` above make
// three passes over LDS scores with ~8 workgroup barriers; at decode lengths the launch is pure latency, so here
// every (wave, 16-lane group) streams its own positions with an online softmax (running max m, sum l, 8 output
// dims per lane) and the 16 partial states merge once through LDS.  Same F32 math on the same half-rounded K/V; the
// summation order differs (|d out| ~1e-6).  The token being decoded comes from LDS (kx/vx), not from the cache row
// another workgroup is writing.
// The launch is a chain of memory round trips (position -> cache rows -> next rows ...), and the walk is arranged around it
// (round 2, "v3": 6.7 -> 5.1 us per layer at position 128, 11.8 -> 7.4 at 320, 97 -> 49 at 4095; with 8 splits 21.7 -> 15.9):
//   * nothing that can be requested without the position waits for it: q, k, v, the frequencies and the first four cache
//     rows of every position group (row indices clamped to the cache, validity applied later) are in flight before *d_pos
//     is consumed;
//   * four positions per group are in flight instead of one (the next four are requested as soon as the current four are
//     unpacked, under a uniform branch; rows past the position are fetched and ignored, so no load is predicated per lane);
//   * the token being decoded is taken by its group after the loop (its place in that group's order);
//   * RoPE of q, RoPE of k and the conversion of v run on different waves, sin and cos share one argument reduction, and the
//     new cache row is stored at the very end (a store in front of the walk sits in the same in-order counter as the row loads);
//   * the merge computes each group's weight once.
// SPLIT: workgroup (head, sp) of nsplit takes the positions sp * G + g + j * nsplit * G of group g and leaves its un-normalised
// state (acc[hd], m, l) in `output` = part[head][sp] for attention_split_combine_kernel; otherwise nsplit = 1 and `output` is the
// head's normalised result.
// ---------------------------------------------------------------------------------------------
template <int LPR, int D, bool SPLIT, bool MERGE = false>   // MERGE: the partial state is written through (attention_merge.hip.h)
__device__ __forceinline__ void attention_decode_walk(
    float* __restrict__ output, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, const int* __restrict__ d_pos, const float* __restrict__ inv_freq,
    const int n_heads, const int n_kv_heads, const int hd, const int max_seq, const float scale, const float theta, const float fscale,
    const int head, const int sp, const int nsplit) {
    constexpr int PPW = 64 / LPR, NW = 4, G = NW * PPW;   // D: positions in flight per group
    constexpr float EMPTY = -3.0e38f;   // running maximum of a group that has seen nothing (finite: exp(EMPTY - x) = 0, EMPTY - EMPTY = 0)
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int group = n_heads / n_kv_heads, kv_head = head / group;
    const int stepG = nsplit * G, first = sp * G;   // this workgroup's positions: first + g + j * stepG
    float* qs = lds;              // [hd] post-RoPE query; after the walk: [G] merge weights
    float* kx = qs + hd;          // [hd] post-RoPE key of this token, rounded through half
    float* vx = kx + hd;          // [hd] value of this token, rounded through half
    float* ms = vx + hd;          // [G] running maxima
    float* ls = ms + G;           // [G] running sums
    float* accs = ls + G;         // [G][hd]
    const int half_dim = hd / 2;
    const size_t stride = (size_t)n_kv_heads * hd;
    const int sub = lane / LPR, part_i = lane % LPR, g = wave * PPW + sub;
    const uint16_t* kbase = kc + (size_t)kv_head * hd + 8 * part_i;
    const uint16_t* vbase = vc + (size_t)kv_head * hd + 8 * part_i;
    const int pmax = max_seq - 1;

    // this thread's share of the new token: wave 0 rotates q, wave 1 rotates and stores k, waves 2-3 store v (hd <= 256)
    const int ri = tid & 63, role = tid >> 6;
    float in_a = 0.0f, in_b = 0.0f, in_c = 0.0f, in_d = 0.0f, freq = 0.0f;
    const bool rot = role < 2 && ri < half_dim;
    if (rot) {   // pairs (ri, ri + hd/2) and, for hd = 256, (ri + 64, ri + 64 + hd/2)
        const float* src = role == 0 ? q + (size_t)head * hd : k + (size_t)kv_head * hd;
        in_a = src[ri]; in_b = src[ri + half_dim];
        freq = inv_freq ? inv_freq[ri] : 1.0f / (float)pow((double)theta, (double)((2.0f * ri) / hd));
        if (half_dim > 64) { in_c = src[ri + 64]; in_d = src[ri + 64 + half_dim]; }
    }
    float vin0 = 0.0f, vin1 = 0.0f;
    const int vi = tid - 128;
    if (role >= 2) {
        if (vi < hd) vin0 = v[(size_t)kv_head * hd + vi];
        if (vi + 128 < hd) vin1 = v[(size_t)kv_head * hd + vi + 128];
    }

    // (after the loads RoPE waits for: a CU serves its requests roughly in order)
    // Rows are addressed by 32-bit byte offsets inside the layer's cache (max_seq * row bytes < 4 GiB: host-checked), advanced by a constant
    // per batch and clamped to the last row: an add and a min per row where the 64-bit form spent a quarter-rate multiply and a 64-bit
    // multiply-add (36 of the walk's ~250 issue slots per batch of 4 positions).
    const unsigned row_bytes = (unsigned)stride * 2u, off_max = (unsigned)pmax * row_bytes, adv = (unsigned)(stepG * D) * row_bytes;
    const char* kb = reinterpret_cast<const char*>(kbase);
    const char* vb = reinterpret_cast<const char*>(vbase);
    unsigned roff[D];
    u32x4 kraw[D], vraw[D];
#pragma unroll
    for (int d = 0; d < D; ++d) {
        roff[d] = min((unsigned)(first + g + stepG * d) * row_bytes, off_max);
        kraw[d] = *reinterpret_cast<const u32x4*>(kb + roff[d]);
        vraw[d] = *reinterpret_cast<const u32x4*>(vb + roff[d]);
    }
    const int pos = *d_pos;
    const size_t cache_row = (size_t)pos * stride + (size_t)kv_head * hd;
    const bool writer = (head % group == 0) && sp == 0 && pos < max_seq;
    // the new cache row is stored at the very END of the kernel (values kept in registers): a store in front of the walk would
    // sit in the same in-order counter as the row loads and make the first wait of the walk a wait for its acknowledgement
    uint16_t st_h[4] = {0, 0, 0, 0};
    if (rot) {
        // reference rotary.cu:46-60; inv_freq (engine) holds 1/powf(theta, 2i/hd) computed once on the host
        auto rotate = [&](const int i, const float a, const float b, const float f, uint16_t& ha, uint16_t& hb) {
            const float angle = pos * f * fscale;
            float c, sn;
            sincosf(angle, &sn, &c);   // one argument reduction; bit-identical to sinf / cosf on gfx950 (tools/micro/sincos_check.hip)
            float ra, rb;
            rope_rotate(a, b, c, sn, ra, rb);
            if (role == 0) { qs[i] = ra; qs[i + half_dim] = rb; }
            else {
                ha = f2h(ra); hb = f2h(rb);   // attention.cu:338 (__float2half, RNE)
                kx[i] = h2f(ha); kx[i + half_dim] = h2f(hb);
            }
        };
        rotate(ri, in_a, in_b, freq, st_h[0], st_h[1]);
        if (half_dim > 64) {
            const int i2 = ri + 64;
            const float f2 = inv_freq ? inv_freq[i2] : 1.0f / (float)pow((double)theta, (double)((2.0f * i2) / hd));
            rotate(i2, in_c, in_d, f2, st_h[2], st_h[3]);
        }
    }
    if (role >= 2) {
        if (vi < hd) { st_h[0] = f2h(vin0); vx[vi] = h2f(st_h[0]); }
        if (vi + 128 < hd) { st_h[1] = f2h(vin1); vx[vi + 128] = h2f(st_h[1]); }
    }
    __syncthreads();

    float qreg[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) qreg[j] = qs[8 * part_i + j];
    float m = EMPTY, l = 0.0f, acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.0f;
    // NP positions of the group's walk as ONE online-softmax update: their scores first, then one rescale of the running state by
    // exp(m - new max) and NP weights -- NP + 1 exponentials instead of 2 NP, and the hardware exponential (v_exp_f32 on x * log2 e,
    // ~1 ulp; the reference's CUDA build evaluates expf the same way under --use_fast_math, CMakeLists.txt:20) instead of libm's
    // ~15-instruction expf: the walk is bound by its VALU work (one wave per SIMD), 75 -> 45 instructions per position and head
    // (round 3; measured: 8 rows in flight or 8-wave workgroups instead changed nothing, profiles/r03_attention_kv_head_form.txt).
    // Invalid positions (past the token, or a clamped row) are exact no-ops.
    // MASKED = false: every one of the np positions exists (all batches but the last): no selects.  V stays packed (two halves per dword).
    auto batch = [&](const float (*kf)[8], const u32x4* vr, const bool* valid, const int np, const bool masked) {
        float sc[D];
        float mn = m;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (d >= np) { sc[d] = EMPTY; continue; }
            float t = 0.0f;
#pragma unroll
            for (int j = 0; j < 8; ++j) t = fmaf(qreg[j], kf[d][j], t);
            t = group_sum<LPR>(t) * scale;
            sc[d] = (!masked || valid[d]) ? t : EMPTY;
            mn = fmaxf(mn, sc[d]);
        }
        const float a = __expf(m - mn);
        l *= a;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] *= a;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            if (d >= np) continue;
            const float pw = (!masked || valid[d]) ? __expf(sc[d] - mn) : 0.0f;
            l += pw;
            pv_update(acc, vr[d], pw);
        }
        m = mn;
    };
    auto walk_batch = [&](const int base, const bool masked) {
        float kf[D][8];
        u32x4 vr[D];
        bool valid[D];
#pragma unroll
        for (int d = 0; d < D; ++d) {
            valid[d] = base + g + stepG * d < pos;
            vr[d] = vraw[d];
            if (masked && !valid[d]) vr[d] = u32x4{0u, 0u, 0u, 0u};   // rows past the position hold anything (0 * NaN)
            unpack8(kraw[d], kf[d]);
        }
        __builtin_amdgcn_sched_barrier(0);   // the ring registers are free: the next batch may land in them
        if (base + stepG * D < pos) {   // uniform: another batch follows
#pragma unroll
            for (int d = 0; d < D; ++d) {
                roff[d] = min(roff[d] + adv, off_max);
                kraw[d] = *reinterpret_cast<const u32x4*>(kb + roff[d]);
                vraw[d] = *reinterpret_cast<const u32x4*>(vb + roff[d]);
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        batch(kf, vr, valid, D, masked);
    };
    int base = first;
    for (; base + stepG * (D - 1) + G <= pos; base += stepG * D) walk_batch(base, false);   // whole batches: every position of every group exists
    if (base < pos) walk_batch(base, true);                                                  // (uniform) the last one, masked
    {   // the token being decoded: from LDS (another workgroup is writing its cache row), by the group whose turn it is
        float kf[D][8];
        u32x4 vr[D];
        bool valid[D];
#pragma unroll
        for (int j = 0; j < 8; ++j) kf[0][j] = kx[8 * part_i + j];
        {   // vx holds the value rounded through half: its half bits again (exact)
            const float* vxp = vx + 8 * part_i;
            vr[0].x = (uint32_t)f2h(vxp[0]) | ((uint32_t)f2h(vxp[1]) << 16); vr[0].y = (uint32_t)f2h(vxp[2]) | ((uint32_t)f2h(vxp[3]) << 16);
            vr[0].z = (uint32_t)f2h(vxp[4]) | ((uint32_t)f2h(vxp[5]) << 16); vr[0].w = (uint32_t)f2h(vxp[6]) | ((uint32_t)f2h(vxp[7]) << 16);
        }
        valid[0] = first + g == pos % stepG;
        batch(kf, vr, valid, 1, true);
    }
    if (part_i == 0) { ms[g] = m; ls[g] = l; }
#pragma unroll
    for (int j = 0; j < 8; ++j) accs[g * hd + 8 * part_i + j] = acc[j];
    __syncthreads();
    float M = ms[0];
    for (int i = 1; i < G; ++i) M = fmaxf(M, ms[i]);
    if (tid < G) qs[tid] = expf(ms[tid] - M);   // 0 for groups that saw no position
    __syncthreads();
    for (int d = tid; d < hd; d += blockDim.x) {
        float L = 0.0f, o = 0.0f;
        for (int i = 0; i < G; ++i) {
            const float w = qs[i];
            L = fmaf(w, ls[i], L);
            o = fmaf(w, accs[i * hd + d], o);
        }
        if constexpr (SPLIT) {
            att_part_store<MERGE>(output + d, o);
            if (d == 0) { att_part_store<MERGE>(output + hd, M); att_part_store<MERGE>(output + hd + 1, L); }
        } else {
            output[(size_t)head * hd + d] = o / L;
        }
    }
    if (writer) {
        if (role == 1 && rot) {
            kc[cache_row + ri] = st_h[0]; kc[cache_row + ri + half_dim] = st_h[1];
            if (half_dim > 64) { kc[cache_row + ri + 64] = st_h[2]; kc[cache_row + ri + 64 + half_dim] = st_h[3]; }
        }
        if (role >= 2) {
            if (vi < hd) vc[cache_row + vi] = st_h[0];
            if (vi + 128 < hd) vc[cache_row + vi + 128] = st_h[1];
        }
    }
}

// the merge of one head's nsplit states by a workgroup of 128 threads: workgroup `block` of `nblocks` (= n_heads) of its row
__device__ __forceinline__ void attention_split_combine_head(float* __restrict__ output, const float* __restrict__ part, int hd, int nsplit,
                                                             int n_kv_heads, const int block, const int nblocks) {
    // One workgroup per head, ONE memory round trip for everything: thread s requests split s's (m, l), then every thread requests its
    // output element of up to 32 splits at once; the weights exp(m_s - M) go through LDS while those loads are in flight; the sums run in
    // split order.  Every loop over the splits is unrolled in blocks of 32 over tables padded with exact no-ops (weight 0, l 0, m -inf): a
    // rolled loop pays an LDS round trip per split and sum -- the kernel trace of the 3.9K-context decode showed this launch at 5.1 us,
    // three quarters of it in three such loops over 32 splits (profiles/r04_rocprofv3_kernel_trace_8b_q8_0_ctx3900.txt, first pass).
    // (Round 3 walked the splits in two rolled loops of dependent GLOBAL loads.)  Workgroup b serves head
    // (b % n_kv_heads) * group + b / n_kv_heads: on the XCD (b % 8) whose L2 the partial states of that KV head were written through.
    constexpr int B = 32;
    __shared__ __attribute__((aligned(16))) float wsh[1024], lsh[1024];
    const int group = nblocks / n_kv_heads;
    const int head = (block % n_kv_heads) * group + block / n_kv_heads, tid = threadIdx.x;
    const float* ph = part + (size_t)head * nsplit * (hd + 2);
    const int n32 = (nsplit + B - 1) / B * B;   // <= 1024 (host-checked)
    float mreg[8], lreg[8];                      // thread t: splits t, t + 128 ...
#pragma unroll
    for (int u = 0; u < 8; ++u) {
        mreg[u] = -INFINITY; lreg[u] = 0.0f;
        if (128 * u < nsplit) {   // (uniform)
            const int s0 = tid + 128 * u;
            const float* ps = ph + (size_t)min(s0, nsplit - 1) * (hd + 2) + hd;
            const float mv = ps[0], lv = ps[1];
            if (s0 < nsplit) { mreg[u] = mv; lreg[u] = lv; }
        }
    }
    const int d0 = min(tid, hd - 1);
    float v0[B];
#pragma unroll
    for (int u = 0; u < B; ++u) v0[u] = ph[(size_t)min(u, nsplit - 1) * (hd + 2) + d0];
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < 8; ++u)
        if (tid + 128 * u < n32) { wsh[tid + 128 * u] = mreg[u]; lsh[tid + 128 * u] = lreg[u]; }
    __syncthreads();
    float M = -INFINITY;
    for (int s0 = 0; s0 < n32; s0 += B) {
#pragma unroll
        for (int u = 0; u < B; ++u) M = fmaxf(M, wsh[s0 + u]);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < 8; ++u)   // (a split that saw no position: m = -inf, or the walk's finite EMPTY: weight 0 either way)
        if (tid + 128 * u < n32) wsh[tid + 128 * u] = (mreg[u] == -INFINITY) ? 0.0f : expf(mreg[u] - M);
    __syncthreads();
    float L = 0.0f;
    for (int s0 = 0; s0 < n32; s0 += B) {
#pragma unroll
        for (int u = 0; u < B; ++u) L = fmaf(wsh[s0 + u], lsh[s0 + u], L);   // split order, like the output sums
    }
    for (int d = tid; d < hd; d += blockDim.x) {
        float o = 0.0f;
        for (int s0 = 0; s0 < n32; s0 += B) {
            float v[B];
            if (s0 == 0 && d == d0) {
#pragma unroll
                for (int u = 0; u < B; ++u) v[u] = v0[u];
            } else {
#pragma unroll
                for (int u = 0; u < B; ++u) v[u] = ph[(size_t)min(s0 + u, nsplit - 1) * (hd + 2) + d];
            }
#pragma unroll
            for (int u = 0; u < B; ++u) o = fmaf(wsh[s0 + u], v[u], o);   // (past the last split: weight 0 x a finite duplicate)
        }
        output[(size_t)head * hd + d] = o / L;
    }
}

}  // namespace ntk
