// attention_fp8_decode.hip.h -- decode attention over the FP8 (OCP E4M3) KV cache as a DEVICE FUNCTION (kernel: attention_fp8.hip), with the
// encoder and the E4M3 -> F16 conversion the store and image kernels of that file share.  Format, layout and exactness: attention_fp8.hip.
#pragma once
#include "common.hip.h"

namespace ntk {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

// ---- the encoder: F32 -> E4M3 by v_cvt_pk_fp8_f32 (RNE).  The saturation is done in F32 by selects, so it does not hang on the mode register's
//      overflow bit: every |x| > 448 (infinities included) becomes +-448, a NaN fails both comparisons and reaches the instruction as it is. ----
__device__ __forceinline__ float fp8_sat(const float x) {
    const float a = x > 448.0f ? 448.0f : x;
    return a < -448.0f ? -448.0f : a;
}
__device__ __forceinline__ uint8_t fp8_encode(const float x) {
    const float s = fp8_sat(x);
    return (uint8_t)(__builtin_amdgcn_cvt_pk_fp8_f32(s, s, 0, false) & 0xFF);
}
__device__ __forceinline__ uint32_t fp8_encode4(const float a, const float b, const float c, const float d) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_sat(a), fp8_sat(b), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(fp8_sat(c), fp8_sat(d), w, true);
    return (uint32_t)w;
}

// ---- eight E4M3 bytes -> eight halves, exactly (every E4M3 value, its subnormals from 2^-9 on included, is a NORMAL half): four
//      v_cvt_scalef32_pk_f16_fp8 with the unit scale -- one instruction per two elements, no F32 detour.  A NaN byte gives a NaN half. ----
__device__ __forceinline__ u32x4 fp8_cvt8(const u32x2 raw) {
    u32x4 r;
    r.x = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)raw.x, 1.0f, false));
    r.y = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)raw.x, 1.0f, true));
    r.z = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)raw.y, 1.0f, false));
    r.w = __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_f16_fp8((int)raw.y, 1.0f, true));
    return r;
}

__device__ __forceinline__ void fp8_split8(const float (&x)[8], f16x8& hi, f16x8& lo) {   // x = hi + lo, as attention_mfma_decode.hip.h's am_split8
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const _Float16 h = (_Float16)x[e];
        hi[e] = h;
        lo[e] = (_Float16)(x[e] - (float)h);
    }
}

// =================================================================================================================================
// Decode attention over the FP8 cache.  One workgroup of 256 threads per (KV head, split); the positions 0 .. pos in chunks of 32 cache
// rows, chunk c to wave (c mod W) of the W = 4 nsplit waves of the KV head; every cache byte read once, rows requested before the position
// is known (addresses do not depend on it) and masked by selects -- rows past the position may hold anything, NaN bytes included: a K row
// only reaches the scores of its own key, which the select replaces; a V row is zeroed as bytes before it is converted.
//   K: lane (i, g) loads dims 32c + 8g .. +7 of key 16 mt + i: 8 bytes, four conversions, and the eight halves ARE the A operand of
//      S^T[key][head] = K . (q scale)^T (v_mfma_f32_16x16x32_f16, q as an F16 value + the F16 rounding of the rest).
//   V: lane p = lane + 64 n -> piece pc = p & 15 (8 dims = 8 bytes) of rows 4 rg .. + 3, rg = p >> 4; converted in registers, then the
//      half-pair transposes and the swizzled wave-private V^T image [128 dims][40 halves] of the F16 kernel (attention_mfma_decode.hip.h),
//      whose 8-byte operand reads do not conflict -- no byte transposes, no 4 x 4 byte shuffles through LDS.
// A chunk costs a lane 64 conversions (32 rows x 128 dims x 2 sides / 64 lanes / 2 per instruction), nothing else beyond the F16 kernel,
// and half the F16 kernel's row registers (32 dwords in flight instead of 64).
// The token being decoded: RoPE of the group's queries by all workgroups; RoPE of k and the encoding of k and v (from the F32 values) by the
// workgroup whose wave owns chunk pos / 32, which takes the new row from LDS and stores it at the end -- the only cache bytes written.
// A split whose waves own no chunk up to pos / 32 leaves an empty state (m = -inf, l = 0: weight 0 in the merge).
// Output: un-normalised partial states part[head][split] = (acc[128], m, l) for attention_split_combine_kernel.
// =================================================================================================================================
constexpr int F8_HD = 128;
constexpr int F8_CK = 32;                       // cache rows per chunk
constexpr int F8_VP = 40;                       // halves per V^T row in LDS (80 B: the 8-byte operand reads of 32 lanes cover 64 banks)
constexpr int F8_WAVE_LDS = F8_HD * F8_VP * 2;  // 10240 B per wave: V^T of its chunk; afterwards its partial output [head][128] floats

__device__ __forceinline__ void attention_decode_fp8_row(
    float* __restrict__ part, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, uint8_t* __restrict__ kc,
    uint8_t* __restrict__ vc, const int* __restrict__ d_pos, const float* __restrict__ inv_freq, const int n_heads, const int n_kv_heads,
    const int max_seq, const float scale, const float theta, const float fscale, const int kv_head, const int sp, const int nsplit) {
    // one LDS object: [queries 16 x 128 f32][new k row, new v row as bytes][4 wave regions][m, l of 4 waves x 16 heads]
    __shared__ __attribute__((aligned(16))) uint8_t smem[16 * F8_HD * 4 + 2 * F8_HD + 4 * F8_WAVE_LDS + 2 * 64 * 4];
    float* qs = reinterpret_cast<float*>(smem);
    uint8_t* knew = smem + 16 * F8_HD * 4;
    uint8_t* vnew = knew + F8_HD;
    uint8_t* wl0 = vnew + F8_HD;
    float* ms = reinterpret_cast<float*>(wl0 + 4 * F8_WAVE_LDS);
    float* ls = ms + 64;

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int i = lane & 15, g = lane >> 4;
    const int group = n_heads / n_kv_heads;               // query heads per KV head (<= 16: host-checked)
    const int W = 4 * nsplit, gw = 4 * sp + wave;
    const unsigned row_bytes = (unsigned)n_kv_heads * F8_HD;
    const uint8_t* kb = kc + (size_t)kv_head * F8_HD;
    const uint8_t* vb = vc + (size_t)kv_head * F8_HD;
    const unsigned last_row = (unsigned)(max_seq - 1);    // (a row index is clamped to it: no address leaves the layer buffer)

    // ---- a chunk's rows (32-bit byte offsets: host-checked) ----
    u32x2 kraw[2][4], vraw[2][4];
    auto request = [&](const int chunk) {
        const unsigned r0 = (unsigned)chunk * F8_CK;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const unsigned off = min(r0 + 16u * mt + (unsigned)i, last_row) * row_bytes + 8u * g;
#pragma unroll
            for (int c = 0; c < 4; ++c) kraw[mt][c] = *reinterpret_cast<const u32x2*>(kb + off + 32u * c);
        }
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int p = lane + 64 * n;
            const unsigned rbase = r0 + 4u * (unsigned)(p >> 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) vraw[n][r] = *reinterpret_cast<const u32x2*>(vb + min(rbase + r, last_row) * row_bytes + 8u * (p & 15));
        }
    };
    // the token's own inputs first (attention_mfma_decode.hip.h: a CU returns its loads in request order)
    const int ri = tid & 63;
    float qa[4], qb[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int n = (tid >> 6) + 4 * u;
        qa[u] = qb[u] = 0.0f;
        if (n < group) {
            const float* src = q + ((size_t)kv_head * group + n) * F8_HD;
            qa[u] = src[ri]; qb[u] = src[ri + 64];
        }
    }
    float ka_in = 0.0f, kb_in = 0.0f, v_in = 0.0f;
    if (tid < 64) { const float* src = k + (size_t)kv_head * F8_HD; ka_in = src[tid]; kb_in = src[tid + 64]; }
    else if (tid >= 128) v_in = v[(size_t)kv_head * F8_HD + tid - 128];
    const float freq = inv_freq ? inv_freq[ri] : 1.0f / (float)pow((double)theta, (double)((2.0f * ri) / F8_HD));
    const int pos = *d_pos;
    __builtin_amdgcn_sched_barrier(0);   // (the compiler may not hoist the cache rows above the token's loads)
    request(gw);
    __builtin_amdgcn_sched_barrier(0);

    // ---- the token being decoded: RoPE (reference rotary.cu:46-60), then the encoder ----
    float rc, rs;
    {
        const float angle = pos * freq * fscale;
        sincosf(angle, &rs, &rc);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int n = (tid >> 6) + 4 * u;
        if (n < group) rope_rotate(qa[u], qb[u], rc, rs, qs[n * F8_HD + ri], qs[n * F8_HD + ri + 64]);
    }
    const int own_chunk = pos / F8_CK;
    const bool owner_wg = ((own_chunk % W) >> 2) == sp;   // (uniform) the chunk of the token belongs to a wave of this workgroup
    const bool writer = owner_wg && pos < max_seq;
    uint8_t st_b[2] = {0, 0};
    if (owner_wg) {
        if (tid < 64) {                                    // key pair (tid, tid + 64)
            float ra, rb;
            rope_rotate(ka_in, kb_in, rc, rs, ra, rb);
            st_b[0] = fp8_encode(ra); st_b[1] = fp8_encode(rb);
            knew[tid] = st_b[0]; knew[tid + 64] = st_b[1];
        } else if (tid >= 128) {                           // value element tid - 128
            st_b[0] = fp8_encode(v_in);
            vnew[tid - 128] = st_b[0];
        }
    }
    __syncthreads();

    // Q operand: (q * scale) as hi + lo halves; lane (i, g): head i, dims 32c + 8g .. +7.  Heads past the group: zero columns.
    f16x8 qh[4], ql[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float x[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) x[e] = 0.0f;
        if (i < group) {
            const float4 a = *reinterpret_cast<const float4*>(qs + i * F8_HD + 32 * c + 8 * g);
            const float4 b = *reinterpret_cast<const float4*>(qs + i * F8_HD + 32 * c + 8 * g + 4);
            x[0] = a.x * scale; x[1] = a.y * scale; x[2] = a.z * scale; x[3] = a.w * scale;
            x[4] = b.x * scale; x[5] = b.y * scale; x[6] = b.z * scale; x[7] = b.w * scale;
        }
        fp8_split8(x, qh[c], ql[c]);
    }

    f32x4 o[8];   // O^T: dims 16 ht + 4g + e of head i
#pragma unroll
    for (int ht = 0; ht < 8; ++ht) o[ht] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    float m_run = -INFINITY, l_run = 0.0f;
    uint16_t* vt = reinterpret_cast<uint16_t*>(wl0 + wave * F8_WAVE_LDS);   // this wave's V^T image [128 dims][F8_VP]
    const int nchunks = own_chunk + 1;

    for (int chunk = gw; chunk < nchunks; chunk += W) {
        const int r0 = chunk * F8_CK;
        const bool last = chunk == own_chunk;   // (uniform) holds the token being decoded, and rows past it
        u32x2 kr[2][4], vr[2][4];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int c = 0; c < 4; ++c) { kr[mt][c] = kraw[mt][c]; vr[mt][c] = vraw[mt][c]; }
        if (last) {   // the new row from LDS; V rows past it zeroed as bytes -- their scores are masked below
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                if (r0 + 16 * mt + i == pos) {
#pragma unroll
                    for (int c = 0; c < 4; ++c) kr[mt][c] = *reinterpret_cast<const u32x2*>(knew + 32 * c + 8 * g);
                }
            }
#pragma unroll
            for (int n = 0; n < 2; ++n) {
                const int p = lane + 64 * n;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int key = r0 + 4 * (p >> 4) + r;
                    if (key == pos) vr[n][r] = *reinterpret_cast<const u32x2*>(vnew + 8 * (p & 15));
                    if (key > pos) vr[n][r] = u32x2{0u, 0u};
                }
            }
        }
        __builtin_amdgcn_sched_barrier(0);
        if (chunk + W < nchunks) request(chunk + W);   // (uniform) the ring registers are free: the next chunk may land in them
        __builtin_amdgcn_sched_barrier(0);

        // ---- V^T image: convert, then per head_dim value the four rows' halves as one 8-byte store; key group (4 rows) rg of dim d sits at
        //      column group rg ^ ((d >> 3) & 7) (attention_mfma_decode.hip.h) ----
#pragma unroll
        for (int n = 0; n < 2; ++n) {
            const int p = lane + 64 * n, pc = p & 15, rg = p >> 4;
            const int col = 4 * (rg ^ (pc & 7));
            const u32x4 h0 = fp8_cvt8(vr[n][0]), h1 = fp8_cvt8(vr[n][1]), h2 = fp8_cvt8(vr[n][2]), h3 = fp8_cvt8(vr[n][3]);
#pragma unroll
            for (int e2 = 0; e2 < 4; ++e2) {   // dword e2 of a piece: dims 8 pc + 2 e2 (low half) and 8 pc + 2 e2 + 1 (high half)
                const uint32_t w0 = h0[e2], w1 = h1[e2], w2 = h2[e2], w3 = h3[e2];
                const u32x2 lo = {__builtin_amdgcn_perm(w1, w0, 0x05040100u), __builtin_amdgcn_perm(w3, w2, 0x05040100u)};
                const u32x2 hi = {__builtin_amdgcn_perm(w1, w0, 0x07060302u), __builtin_amdgcn_perm(w3, w2, 0x07060302u)};
                *reinterpret_cast<u32x2*>(vt + (8 * pc + 2 * e2) * F8_VP + col) = lo;
                *reinterpret_cast<u32x2*>(vt + (8 * pc + 2 * e2 + 1) * F8_VP + col) = hi;
            }
        }

        // ---- S^T = K . Q^T: lane (i, g): head i, keys r0 + 16 mt + 4g + e ----
        f32x4 s[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            f32x4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const f16x8 a = __builtin_bit_cast(f16x8, fp8_cvt8(kr[mt][c]));
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, qh[c], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, ql[c], acc, 0, 0, 0);
            }
            s[mt] = acc;
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
        f16x8 ph, pl;
        fp8_split8(pv, ph, pl);
        l_tile += __shfl_xor(l_tile, 16, 64);
        l_tile += __shfl_xor(l_tile, 32, 64);
        l_run = l_run * alpha + l_tile;
        m_run = m_new;

        // ---- O^T = alpha O^T + V^T . P^T ----
#pragma unroll
        for (int ht = 0; ht < 8; ++ht) {
            const int d = 16 * ht + i, sw = (d >> 3) & 7;
            const uint16_t* vrow = vt + d * F8_VP;
            const u32x2 v0 = *reinterpret_cast<const u32x2*>(vrow + 4 * (g ^ sw));          // keys 4g .. 4g+3
            const u32x2 v1 = *reinterpret_cast<const u32x2*>(vrow + 4 * ((4 + g) ^ sw));    // keys 16 + 4g .. 16 + 4g+3
            const f16x8 va = __builtin_bit_cast(f16x8, u32x4{v0.x, v0.y, v1.x, v1.y});
            f32x4 acc = o[ht] * alpha;
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, ph, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pl, acc, 0, 0, 0);
            o[ht] = acc;
        }
    }

    // ---- merge the four waves (un-normalised states), write part[head][sp] = (acc[128], m, l) ----
    float* mine = reinterpret_cast<float*>(wl0 + wave * F8_WAVE_LDS);   // [head][128] (the wave's own LDS reads are behind it: in order)
    if (i < group) {
#pragma unroll
        for (int ht = 0; ht < 8; ++ht) *reinterpret_cast<f32x4*>(mine + i * F8_HD + 16 * ht + 4 * g) = o[ht];
        if (g == 0) { ms[wave * 16 + i] = m_run; ls[wave * 16 + i] = l_run; }
    }
    __syncthreads();
    for (int idx = tid; idx < group * F8_HD; idx += 256) {
        const int n = idx >> 7, d = idx & (F8_HD - 1);
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
                acc = fmaf(wgt, reinterpret_cast<const float*>(wl0 + w * F8_WAVE_LDS)[n * F8_HD + d], acc);
            }
        }
        float* out = part + (((size_t)kv_head * group + n) * nsplit + sp) * (F8_HD + 2);
        out[d] = acc;
        if (d == 0) { out[F8_HD] = M; out[F8_HD + 1] = L; }
    }
    if (writer) {   // the new cache row, at the very end (attention.hip: a store in front of the walk delays the first row)
        const size_t cache_row = (size_t)pos * n_kv_heads * F8_HD + (size_t)kv_head * F8_HD;
        if (tid < 64) { kc[cache_row + tid] = st_b[0]; kc[cache_row + tid + 64] = st_b[1]; }
        else if (tid >= 128) vc[cache_row + tid - 128] = st_b[0];
    }
}

}  // namespace ntk
