// attention_q8_decode.hip.h -- decode attention over the 8-bit (Q8_0) KV cache as a DEVICE FUNCTION, shared by the single-row kernel
// (attention_decode_q8_kernel) and the batched one (attention_batch_q8_kernel), both in attention_q8.hip -- the way attention_decode.hip.h and
// attention_mfma_decode.hip.h serve attention_batch.hip: one body, so a batched row is the single-row launch's bits.  The quantiser and the
// int8 -> F16 helpers live here too (the store kernels of attention_q8.hip use the same quantiser).  Format, layout and exactness: attention_q8.hip.
#pragma once
#include "common.hip.h"

namespace ntk {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// ---- the quantiser: one element per lane, a block = 32 consecutive lanes (an aligned half of a wave); all 32 lanes must be active ----
__device__ __forceinline__ void q8_quantise_lane(const float x, int8_t& q, uint16_t& dh) {
    float amax = fabsf(x);
#pragma unroll
    for (int m = 16; m >= 1; m >>= 1) amax = fmaxf(amax, __shfl_xor(amax, m, 64));
    const float d = amax / 127.0f;                 // IEEE division (-fhip-fp32-correctly-rounded-divide-sqrt: Makefile)
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    float t = x * id;
    t = t != t ? 0.0f : t;                         // 0 * inf (subnormal amax): pinned to 0
    t = fminf(fmaxf(t, -127.0f), 127.0f);          // inf (same case): pinned to +-127; |x * id| of a defined case rounds to <= 127 anyway
    q = (int8_t)(int)roundf(t);                    // ties away from zero
    dh = f2h(d);
}

// four int8 (biased: w = raw ^ 0x80808080, so a byte is q + 128) -> four F16, exactly: 0x6400 | u is the half 1024 + u, minus 1152
__device__ __forceinline__ void q8_cvt4(const uint32_t w, uint32_t& lo, uint32_t& hi) {
    const f16x2 bias = {(_Float16)1152.0f, (_Float16)1152.0f};
    const f16x2 a = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0x64646464u, w, 0x04010400u)) - bias;
    const f16x2 b = __builtin_bit_cast(f16x2, __builtin_amdgcn_perm(0x64646464u, w, 0x04030402u)) - bias;
    lo = __builtin_bit_cast(uint32_t, a);
    hi = __builtin_bit_cast(uint32_t, b);
}
__device__ __forceinline__ f16x8 q8_cvt8(const u32x2 raw) {
    u32x4 r;
    uint32_t a, b, c, d;
    q8_cvt4(raw.x ^ 0x80808080u, a, b);
    q8_cvt4(raw.y ^ 0x80808080u, c, d);
    r.x = a; r.y = b; r.z = c; r.w = d;
    return __builtin_bit_cast(f16x8, r);
}
__device__ __forceinline__ float h2f_lo(uint32_t w) { return h2f((uint16_t)(w & 0xFFFFu)); }
__device__ __forceinline__ float h2f_hi(uint32_t w) { return h2f((uint16_t)(w >> 16)); }

__device__ __forceinline__ void q8_split8(const float (&x)[8], f16x8& hi, f16x8& lo) {   // x = hi + lo, as attention_mfma.hip's am_split8
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const _Float16 h = (_Float16)x[e];
        hi[e] = h;
        lo[e] = (_Float16)(x[e] - (float)h);
    }
}

// =================================================================================================================================
// Decode attention over the 8-bit cache: attention_decode_kvhead_mfma_kernel (attention_mfma.hip) with int8 rows.  One workgroup per
// (KV head, split); the positions 0 .. pos in chunks of 32 cache rows, chunk c to wave (c mod W) of the W = 4 nsplit waves of the KV head;
// every cache byte read once, rows requested before the position is known (addresses do not depend on it) and masked by selects -- rows
// past the position may hold anything, scale patterns that are NaN or inf included: a K scale only reaches a score that the select replaces,
// a V scale is itself selected to 0 before it touches P.
//   K: lane (i, g) loads dims 32c + 8g .. +7 of key 16 mt + i (8 bytes) = its A operand of block c; S^T accumulates per block, then
//      s += d_c[key] * acc_c with the scales of the accumulator's keys (16 mt + 4g + e), loaded straight in that layout.
//   V: lane -> (16 dims, 4 rows); 4x4 byte transposes into a wave-private image [128 dims][32 keys] (pitch 48 B: the 8-byte operand reads
//      of 32 lanes cover 64 banks; key groups g and g + 4 adjacent), A operand = 8 keys of one dim, converted on the way into the MFMA.
// The token being decoded: RoPE of the group's queries by all workgroups; RoPE of k, quantisation of k and v (from the F32 values) by the
// workgroup whose wave owns chunk pos / 32, which takes the quantised row from LDS and stores it at the end -- the only cache bytes written.
// A split whose waves own no chunk up to pos / 32 (more splits than chunks) leaves an empty state (m = -inf, l = 0: weight 0 in the merge).
// Output: un-normalised partial states part[head][split] = (acc[128], m, l) for attention_split_combine_kernel.
// The caller names the workgroup's (KV head, split, split count): the grid's x, y and y extent in the single-row kernel; a batched caller adds a
// row dimension and passes that row's operands.  Workgroup of 256 threads.
// =================================================================================================================================
constexpr int Q8_HD = 128;
constexpr int Q8_CK = 32;                    // cache rows per chunk
constexpr int Q8_VP = 48;                    // bytes per dim row of the V^T image
constexpr int Q8_WAVE_LDS = 16 * Q8_HD * 4;  // 8192 B per wave: V^T image (6144 B); afterwards the wave's partial output [head][128] floats

__device__ __forceinline__ void attention_decode_q8_row(
    float* __restrict__ part, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    int8_t* __restrict__ kq, uint16_t* __restrict__ ks, int8_t* __restrict__ vq, uint16_t* __restrict__ vs, const int* __restrict__ d_pos,
    const float* __restrict__ inv_freq, const int n_heads, const int n_kv_heads, const int max_seq, const float scale, const float theta,
    const float fscale, const int kv_head, const int sp, const int nsplit) {
    // one LDS object: [queries 16 x 128 f32][rotated k row f32][new row: k quants, v quants, k scales, v scales][4 wave regions][m, l]
    __shared__ __attribute__((aligned(16))) uint8_t smem[16 * Q8_HD * 4 + Q8_HD * 4 + 2 * Q8_HD + 16 + 4 * Q8_WAVE_LDS + 2 * 64 * 4];
    float* qs = reinterpret_cast<float*>(smem);
    float* kf = qs + 16 * Q8_HD;
    uint8_t* knew = smem + 16 * Q8_HD * 4 + Q8_HD * 4;
    uint8_t* vnew = knew + Q8_HD;
    uint16_t* dnew = reinterpret_cast<uint16_t*>(vnew + Q8_HD);   // [0..3] k scales, [4..7] v scales
    uint8_t* wl0 = reinterpret_cast<uint8_t*>(dnew) + 16;
    float* ms = reinterpret_cast<float*>(wl0 + 4 * Q8_WAVE_LDS);
    float* ls = ms + 64;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int group = n_heads / n_kv_heads;               // query heads per KV head (<= 16: host-checked)
    const int W = 4 * nsplit, gw = 4 * sp + wave;
    const unsigned qrow_bytes = (unsigned)n_kv_heads * Q8_HD, srow_bytes = (unsigned)n_kv_heads * 8u;
    const char* kqb = reinterpret_cast<const char*>(kq) + (size_t)kv_head * Q8_HD;
    const char* vqb = reinterpret_cast<const char*>(vq) + (size_t)kv_head * Q8_HD;
    const char* ksb = reinterpret_cast<const char*>(ks) + (size_t)kv_head * 8;
    const char* vsb = reinterpret_cast<const char*>(vs) + (size_t)kv_head * 8;
    const unsigned last_row = (unsigned)(max_seq - 1);

    // ---- a chunk's rows (32-bit byte offsets: host-checked).  K quants: block mt (16 keys), dim block c: the A operand itself.  K / V scales:
    //      the four halves of keys 16 mt + 4g + e (the accumulator's keys).  V quants: lane -> piece pc = lane & 7 (16 dims) of rows 4 rg .. + 3. ----
    u32x2 kraw[2][4], ksc[2][4], vsc[2][4];
    u32x4 vraw[4];
    auto request = [&](const int chunk) {
        const unsigned r0 = (unsigned)chunk * Q8_CK;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const unsigned off = min(r0 + 16u * mt + (unsigned)i, last_row) * qrow_bytes + 8u * g;
#pragma unroll
            for (int c = 0; c < 4; ++c) kraw[mt][c] = *reinterpret_cast<const u32x2*>(kqb + off + 32u * c);
        }
        {
            const unsigned rbase = r0 + 4u * (unsigned)(lane >> 3);
#pragma unroll
            for (int r = 0; r < 4; ++r) vraw[r] = *reinterpret_cast<const u32x4*>(vqb + min(rbase + r, last_row) * qrow_bytes + 16u * (lane & 7));
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const unsigned off = min(r0 + 16u * mt + 4u * g + e, last_row) * srow_bytes;
                ksc[mt][e] = *reinterpret_cast<const u32x2*>(ksb + off);
                vsc[mt][e] = *reinterpret_cast<const u32x2*>(vsb + off);
            }
    };
    // the token's own inputs first (attention_mfma.hip: a CU returns its loads in request order)
    const int ri = tid & 63;
    float qa[4], qb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int n = (tid >> 6) + 4 * u;
        qa[u] = qb[u] = 0.0f;
        if (n < group) {
            const float* src = q + ((size_t)kv_head * group + n) * Q8_HD;
            qa[u] = src[ri]; qb[u] = src[ri + 64];
        }
    }
    float ka_in = 0.0f, kb_in = 0.0f, v_in = 0.0f;
    if (tid < 64) { const float* src = k + (size_t)kv_head * Q8_HD; ka_in = src[tid]; kb_in = src[tid + 64]; }
    else if (tid >= 128) v_in = v[(size_t)kv_head * Q8_HD + tid - 128];
    const float freq = inv_freq ? inv_freq[ri] : 1.0f / (float)pow((double)theta, (double)((2.0f * ri) / Q8_HD));
    const int pos = *d_pos;
    __builtin_amdgcn_sched_barrier(0);   // (the compiler may not hoist the cache rows above the token's loads)
    request(gw);
    __builtin_amdgcn_sched_barrier(0);

    // ---- the token being decoded: RoPE (reference rotary.cu:46-60) ----
    float rc, rs;
    {
        const float angle = pos * freq * fscale;
        sincosf(angle, &rs, &rc);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int n = (tid >> 6) + 4 * u;
        if (n < group) rope_rotate(qa[u], qb[u], rc, rs, qs[n * Q8_HD + ri], qs[n * Q8_HD + ri + 64]);
    }
    const int own_chunk = pos / Q8_CK;
    const bool owner_wg = ((own_chunk % W) >> 2) == sp;   // (uniform) the chunk of the token belongs to a wave of this workgroup
    const bool writer = owner_wg && pos < max_seq;
    if (owner_wg && tid < 64) rope_rotate(ka_in, kb_in, rc, rs, kf[tid], kf[tid + 64]);
    __syncthreads();
    int8_t st_q = 0;
    uint16_t st_d = 0;
    if (owner_wg) {   // thread t: element t & 127 of k (t < 128) or v; a block = 32 consecutive threads
        const float x = tid < 128 ? kf[tid] : v_in;
        q8_quantise_lane(x, st_q, st_d);
        knew[tid] = (uint8_t)st_q;                       // (vnew = knew + 128)
        if ((tid & 31) == 0) dnew[tid >> 5] = st_d;
        __syncthreads();
    }

    // Q operand: (q * scale) as hi + lo halves; lane (i, g): head i, dims 32c + 8g .. +7.  Heads past the group: zero columns.
    f16x8 qh[4], ql[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.0f;
        if (i < group) {
            const float4 a = *reinterpret_cast<const float4*>(qs + i * Q8_HD + 32 * c + 8 * g);
            const float4 b = *reinterpret_cast<const float4*>(qs + i * Q8_HD + 32 * c + 8 * g + 4);
            x[0] = a.x * scale; x[1] = a.y * scale; x[2] = a.z * scale; x[3] = a.w * scale;
            x[4] = b.x * scale; x[5] = b.y * scale; x[6] = b.z * scale; x[7] = b.w * scale;
        }
        q8_split8(x, qh[c], ql[c]);
    }

    f32x4 o[8];   // O^T: dims 16 ht + 4g + e of head i
#pragma unroll
    for (int ht = 0; ht < 8; ++ht) o[ht] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m_run = -INFINITY, l_run = 0.0f;
    uint8_t* vt = wl0 + wave * Q8_WAVE_LDS;   // this wave's V^T image [128 dims][Q8_VP bytes]
    const int nchunks = own_chunk + 1;

    for (int chunk = gw; chunk < nchunks; chunk += W) {
        const int r0 = chunk * Q8_CK;
        const bool last = chunk == own_chunk;   // (uniform) holds the token being decoded, and rows past it
        u32x2 ka[2][4], kd[2][4], vd[2][4];
        u32x4 vv[4];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int c = 0; c < 4; ++c) { ka[mt][c] = kraw[mt][c]; kd[mt][c] = ksc[mt][c]; vd[mt][c] = vsc[mt][c]; }
#pragma unroll
        for (int r = 0; r < 4; ++r) vv[r] = vraw[r];
        if (last) {   // the new row from LDS; rows past it: V quants and V scales zeroed (selects) -- their scores are masked below
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                if (r0 + 16 * mt + i == pos) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) ka[mt][c] = *reinterpret_cast<const u32x2*>(knew + 32 * c + 8 * g);
                }
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int key = r0 + 16 * mt + 4 * g + e;
                    if (key == pos) {
                        kd[mt][e] = *reinterpret_cast<const u32x2*>(dnew);
                        vd[mt][e] = *reinterpret_cast<const u32x2*>(dnew + 4);
                    }
                    if (key > pos) vd[mt][e] = u32x2{0u, 0u};
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int key = r0 + 4 * (lane >> 3) + r;
                if (key == pos) vv[r] = *reinterpret_cast<const u32x4*>(vnew + 16 * (lane & 7));
                if (key > pos) vv[r] = u32x4{0u, 0u, 0u, 0u};
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (chunk + W < nchunks) request(chunk + W);   // (uniform) the ring registers are free: the next chunk may land in them
        __builtin_amdgcn_sched_barrier(0);

        // ---- V^T image: 4x4 byte transposes (rows 4 rg .. + 3 x dims 4j .. + 3 of the piece); key group kg at dword 2 (kg & 3) + (kg >> 2) ----
        {
            const int pc = lane & 7, rg = lane >> 3;
            uint8_t* dst = vt + (16 * pc) * Q8_VP + 4 * (2 * (rg & 3) + (rg >> 2));
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t w0 = vv[0][j], w1 = vv[1][j], w2 = vv[2][j], w3 = vv[3][j];
                const uint32_t a_lo = __builtin_amdgcn_perm(w1, w0, 0x05010400u), a_hi = __builtin_amdgcn_perm(w1, w0, 0x07030602u);
                const uint32_t b_lo = __builtin_amdgcn_perm(w3, w2, 0x05010400u), b_hi = __builtin_amdgcn_perm(w3, w2, 0x07030602u);
                *reinterpret_cast<uint32_t*>(dst + (4 * j + 0) * Q8_VP) = __builtin_amdgcn_perm(b_lo, a_lo, 0x05040100u);
                *reinterpret_cast<uint32_t*>(dst + (4 * j + 1) * Q8_VP) = __builtin_amdgcn_perm(b_lo, a_lo, 0x07060302u);
                *reinterpret_cast<uint32_t*>(dst + (4 * j + 2) * Q8_VP) = __builtin_amdgcn_perm(b_hi, a_hi, 0x05040100u);
                *reinterpret_cast<uint32_t*>(dst + (4 * j + 3) * Q8_VP) = __builtin_amdgcn_perm(b_hi, a_hi, 0x07060302u);
            }
        }

        // ---- S^T = sum over blocks c of d_c[key] * (K_c . Q_c^T): lane (i, g): head i, keys r0 + 16 mt + 4g + e ----
        f32x4 s[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x4 sum = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f16x8 a = q8_cvt8(ka[mt][c]);
                f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qh[c], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, ql[c], acc, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const uint32_t w = c < 2 ? kd[mt][e].x : kd[mt][e].y;
                    sum[e] = fmaf((c & 1) ? h2f_hi(w) : h2f_lo(w), acc[e], sum[e]);
                }
            }
            s[mt] = sum;
        }
        float m_tile = -INFINITY;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                if (last) s[mt][e] = (r0 + 16 * mt + 4 * g + e <= pos) ? s[mt][e] : -INFINITY;   // a select: the row may hold anything
                m_tile = fmaxf(m_tile, s[mt][e]);
            }
        m_tile = fmaxf(m_tile, __shfl_xor(m_tile, 16, 64));
        m_tile = fmaxf(m_tile, __shfl_xor(m_tile, 32, 64));
        const float m_new = fmaxf(m_run, m_tile);          // finite: every chunk holds at least one position <= pos
        const float alpha = __expf(m_run - m_new);         // exp(-inf) = 0 on the wave's first chunk
        float pv[8], l_tile = 0.0f;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            pv[e] = __expf(s[0][e] - m_new);               // keys r0 + 4g + e
            pv[4 + e] = __expf(s[1][e] - m_new);           // keys r0 + 16 + 4g + e
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) l_tile += pv[e];
        l_tile += __shfl_xor(l_tile, 16, 64);
        l_tile += __shfl_xor(l_tile, 32, 64);
        l_run = l_run * alpha + l_tile;
        m_run = m_new;
        // The V scale d = dm * 2^de, both factors exact: the MANTISSA part dm (in [1, 2) for a normal half) is folded into P per dim block -- p * dm
        // has the magnitude of p, so the F16 hi + lo split loses what the F16 kernel's split of p loses and no more -- and the power of two goes onto
        // the V quants of the A operand (q * 2^de is exact in half: 2^-14 <= 2^de <= 2^9, |q| <= 128).  Folding d itself into P would push every
        // weight below 6e-5 / d (about 8e-3 at |v| ~ 1) into the F16 subnormals.
        f16x8 ph[4], pl[4], vfac[4];
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {
            float x[8];
            uint32_t eb[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const u32x2 w2 = vd[e >> 2][e & 3];
                const uint32_t w = blk < 2 ? w2.x : w2.y;
                const uint32_t hb = (blk & 1) ? (w >> 16) : (w & 0xFFFFu);
                uint32_t ex = hb & 0x7C00u;                       // the half 2^de; subnormal d: 2^-14; from 2^10 on (127 * 2^10 overflows half): 2^9
                ex = ex == 0u ? 0x0400u : min(ex, 0x6000u);
                eb[e] = ex;
                const float inv_pow = __uint_as_float((142u - (ex >> 10)) << 23);   // 2^-de
                x[e] = pv[e] * (h2f((uint16_t)hb) * inv_pow);     // (d * 2^-de: exact)
            }
            q8_split8(x, ph[blk], pl[blk]);
            vfac[blk] = __builtin_bit_cast(f16x8, u32x4{eb[0] | (eb[1] << 16), eb[2] | (eb[3] << 16), eb[4] | (eb[5] << 16), eb[6] | (eb[7] << 16)});
        }

        // ---- O^T = alpha O^T + V_q^T . (P d)^T ----
#pragma unroll
        for (int ht = 0; ht < 8; ++ht) {
            const u32x2 vw = *reinterpret_cast<const u32x2*>(vt + (16 * ht + i) * Q8_VP + 8 * g);   // keys 4g .. 4g+3 | 16 + 4g .. 16 + 4g+3
            const f16x8 va = q8_cvt8(vw) * vfac[ht >> 1];
            f32x4 acc = o[ht] * alpha;
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, ph[ht >> 1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pl[ht >> 1], acc, 0, 0, 0);
            o[ht] = acc;
        }
    }

    // ---- merge the four waves (un-normalised states), write part[head][sp] = (acc[128], m, l) ----
    float* mine = reinterpret_cast<float*>(wl0 + wave * Q8_WAVE_LDS);   // [head][128] (the wave's own LDS reads are behind it: in order)
    if (i < group) {
#pragma unroll
        for (int ht = 0; ht < 8; ++ht) *reinterpret_cast<f32x4*>(mine + i * Q8_HD + 16 * ht + 4 * g) = o[ht];
        if (g == 0) { ms[wave * 16 + i] = m_run; ls[wave * 16 + i] = l_run; }
    }
    __syncthreads();
    for (int idx = tid; idx < group * Q8_HD; idx += 256) {
        const int n = idx >> 7, d = idx & (Q8_HD - 1);
        float M = -INFINITY;
#pragma unroll
        for (int w = 0; w < 4; ++w) M = fmaxf(M, ms[w * 16 + n]);
        float L = 0.0f, acc = 0.0f;
        if (M > -INFINITY) {
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const float mw = ms[w * 16 + n];
                const float wgt = mw > -INFINITY ? expf(mw - M) : 0.0f;
                L = fmaf(wgt, ls[w * 16 + n], L);
                acc = fmaf(wgt, reinterpret_cast<const float*>(wl0 + w * Q8_WAVE_LDS)[n * Q8_HD + d], acc);
            }
        }
        float* out = part + (((size_t)kv_head * group + n) * nsplit + sp) * (Q8_HD + 2);
        out[d] = acc;
        if (d == 0) { out[Q8_HD] = M; out[Q8_HD + 1] = L; }
    }
    if (writer) {   // the new cache row, at the very end (attention.hip: a store in front of the walk delays the first row)
        const size_t per = (size_t)n_kv_heads * Q8_HD;
        const size_t e = (size_t)pos * per + (size_t)kv_head * Q8_HD + (tid & 127);
        const size_t b = (size_t)pos * (per / 32) + (size_t)kv_head * 4 + ((tid & 127) >> 5);
        if (tid < 128) { kq[e] = st_q; if ((tid & 31) == 0) ks[b] = st_d; }
        else { vq[e] = st_q; if ((tid & 31) == 0) vs[b] = st_d; }
    }
}

}  // namespace ntk
