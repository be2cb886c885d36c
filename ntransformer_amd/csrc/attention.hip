// attention.hip -- RoPE, KV store and GQA KV-cache attention for gfx950 (wave64).
//
// Replaces: launch_rope (reference src/cuda/rotary.cu:16-140), launch_copy_to_kv_cache, launch_attention_decode,
// launch_attention_prefill (reference src/cuda/attention.cu:108-425).  Same data contract: q/k/v and the
// output are F32, the caches are IEEE half [max_seq][n_kv_heads][head_dim] per layer, math is F32, softmax
// subtracts the row maximum, GQA maps head h to kv head h / (n_heads / n_kv_heads).
//
// What is different from the reference kernels: K and V rows are read 16 bytes per lane (8 halves), head_dim/8
// lanes share one cache row so a wave covers 64/(head_dim/8) positions per instruction; the score dot products
// reduce with wave shuffles instead of a serial per-thread loop; the P.V product is split over positions
// across all waves (the reference walks the positions serially with one thread per output dim).  The
// engine's decode path additionally fuses RoPE + KV store into the attention launch and takes the position
// from device memory so the launch can be replayed from a hipGraph.
// (the decode kernels' device functions: attention_decode.hip.h)
#include "common.hip.h"
#include "attention_merge.hip.h"
#include "attention_decode.hip.h"
#include <cfloat>
#include <cstdlib>

namespace ntk {

// one query of one head over keys 0 .. n_keys - 1 of a cache: out / q point at the (query, head) row; the body of the two kernels below
template <int LPR>
__device__ __forceinline__ void attention_one_query(float* __restrict__ out, const float* __restrict__ q, const uint16_t* __restrict__ kc,
                                                    const uint16_t* __restrict__ vc, const int n_keys, const int head, const int n_heads,
                                                    const int n_kv_heads, const int hd, const float scale) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* qs = lds;                        // [hd]
    float* red = qs + hd;                   // [16]
    float* part = red + 16;                 // [nwaves][hd]
    float* sc = part + (blockDim.x >> 6) * hd;
    for (int d = threadIdx.x; d < hd; d += blockDim.x) qs[d] = q[d];
    __syncthreads();
    attend<LPR>(out, qs, kc, vc, n_keys, nullptr, nullptr, head / (n_heads / n_kv_heads), n_kv_heads, hd, scale, sc, part, red);
}

template <int LPR>
__global__ __launch_bounds__(256) void attention_kernel(float* __restrict__ output, const float* __restrict__ Q,
                                                        const uint16_t* __restrict__ kc, const uint16_t* __restrict__ vc,
                                                        int n_keys_base, int causal, int n_heads, int n_kv_heads, int hd,
                                                        float scale) {
    const int head = blockIdx.x, qi = blockIdx.y;
    const int n_keys = causal ? n_keys_base + qi + 1 : n_keys_base;   // prefill: keys 0..start_pos+qi
    const size_t qoff = ((size_t)qi * n_heads + head) * hd;
    attention_one_query<LPR>(output + qoff, Q + qoff, kc, vc, n_keys, head, n_heads, n_kv_heads, hd, scale);
}

// The SINGLE-ROW segments of a packed prompt pass (ntk_attention_prefill_segments), one launch: workgroup (head, j) is the one query of the j-th of them --
// row row0[j] of Q / output, keys 0 .. start_pos[j] of its own cache -- i.e. attention_kernel's workgroup for a one-row prompt at start_pos[j], the same
// bits.  The table travels in the kernel arguments.
struct SingleRows {
    const uint16_t* k[NTK_ATTN_BATCH_MAX];
    const uint16_t* v[NTK_ATTN_BATCH_MAX];
    int row0[NTK_ATTN_BATCH_MAX], start_pos[NTK_ATTN_BATCH_MAX];
};
template <int LPR>
__global__ __launch_bounds__(256) void attention_single_rows_kernel(float* __restrict__ output, const float* __restrict__ Q, const SingleRows rows,
                                                                    int n_heads, int n_kv_heads, int hd, float scale) {
    const int head = blockIdx.x, j = blockIdx.y;
    const size_t qoff = ((size_t)rows.row0[j] * n_heads + head) * hd;
    attention_one_query<LPR>(output + qoff, Q + qoff, rows.k[j], rows.v[j], rows.start_pos[j] + 1, head, n_heads, n_kv_heads, hd, scale);
}

template <int LPR>
__global__ __launch_bounds__(256) void attention_decode_fused_kernel(
    float* __restrict__ output, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, const int* __restrict__ d_pos, int n_heads, int n_kv_heads,
    int hd, int max_seq, float scale, float theta, float fscale) {
    attention_decode_fused_row<LPR>(output, q, k, v, kc, vc, d_pos, n_heads, n_kv_heads, hd, max_seq, scale, theta, fscale, (int)blockIdx.x);
}


template <int LPR, int D>
__global__ __launch_bounds__(256) void attention_decode_fused_v3_kernel(
    float* __restrict__ output, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, const int* __restrict__ d_pos, const float* __restrict__ inv_freq,
    int n_heads, int n_kv_heads, int hd, int max_seq, float scale, float theta, float fscale) {
    attention_decode_walk<LPR, D, false>(output, q, k, v, kc, vc, d_pos, inv_freq, n_heads, n_kv_heads, hd, max_seq, scale, theta, fscale,
                                         (int)blockIdx.x, 0, 1);
}

// ---------------------------------------------------------------------------------------------
// Split-KV decode attention for long contexts.  One workgroup per head walks the cache serially, so the
// single-pass launch grows with the context (49 us per layer at position 4095, where the whole layer's KV is only 16.8 MB).
// Here `nsplit` workgroups share a head -- grid (n_heads, nsplit), positions interleaved so every split sees the same load --
// and a second launch (attention_split_combine_kernel) merges the nsplit partial states per head.  RoPE + KV store of the new
// token as in the single pass (store: split 0 of the first head of each KV group).  The engine picks single pass / 8 / 16
// splits by position (host side, one hipGraph per regime).
// XCD-aware head order: workgroups are dealt to the 8 XCDs round-robin by linear id and every XCD has its own L2.
// blockIdx.x = i -> kv head i % n_kv_heads: with 8 KV heads (every Llama-3 size) all query heads of a KV head, in all splits,
// run on ONE XCD, so its cache rows leave HBM once instead of once per query head (measured: 4x HBM traffic, 23.6 us per layer
// at position 4095 with the plain order).
// part layout: [n_heads][nsplit][hd + 2] = acc[hd], m, l
// ---------------------------------------------------------------------------------------------
// MERGE: the head's last workgroup to finish merges the nsplit states into output[head] itself (attention_merge.hip.h) -- no combine launch
template <int LPR, int D, bool MERGE>
__global__ __launch_bounds__(256) void attention_decode_split_kernel(
    float* __restrict__ part, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, const int* __restrict__ d_pos, const float* __restrict__ inv_freq,
    int n_heads, int n_kv_heads, int hd, int max_seq, float scale, float theta, float fscale, float* __restrict__ output,
    unsigned* __restrict__ counters) {
    const int group = n_heads / n_kv_heads;
    const int kv_head = blockIdx.x % n_kv_heads, head = kv_head * group + blockIdx.x / n_kv_heads;
    const int sp = blockIdx.y, nsplit = gridDim.y;
    attention_decode_walk<LPR, D, true, MERGE>(part + ((size_t)head * nsplit + sp) * (hd + 2), q, k, v, kc, vc, d_pos, inv_freq, n_heads,
                                               n_kv_heads, hd, max_seq, scale, theta, fscale, head, sp, nsplit);
    if constexpr (MERGE) {
        extern __shared__ __attribute__((aligned(16))) float lds[];   // (the walk's LDS: nothing reads it any more)
        if (!att_merge_arrive(counters + head, nsplit, (int)threadIdx.x, reinterpret_cast<volatile int*>(lds))) return;
        const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
        if (64 * wave < hd)   // (uniform per wave) hd 64: wave 0; 128: waves 0, 1; 256: all four
            att_merge_head_wave<1>(output + (size_t)head * hd, part + (size_t)head * nsplit * (hd + 2), hd, nsplit, lane, 64 * wave + lane);
    }
}

__global__ __launch_bounds__(128) void attention_split_combine_kernel(float* __restrict__ output, const float* __restrict__ part,
                                                                      int hd, int nsplit, int n_kv_heads) {
    attention_split_combine_head(output, part, hd, nsplit, n_kv_heads, (int)blockIdx.x, (int)gridDim.x);
}

// ---------------------------------------------------------------------------------------------
// Prompt attention, flash style (replaces attention_prefill_kernel, reference attention.cu:216-311,
// whose one-block-per-(head, query) form re-reads every K / V row once per query: 32 x 1024 blocks each walking up
// to 1024 keys for a 1024-token prompt).  One workgroup per (head, tile of 32 queries): the keys the tile can see go
// through LDS in tiles of 64 cache rows (K and V, raw halves, 32 KB), every wave owns 8 of the queries and keeps an online
// softmax state (running max, sum, 8 output dims per lane) per query in registers -- the decode kernel's inner loop with
// the cache rows coming from LDS and shared by the 32 queries.  K / V traffic per head falls from T^2 / 2 rows to
// T^2 / 64; no score row in LDS, so no limit on the context.  F32 math on the same half-rounded K / V, causal limit
// start_pos + query index; only the summation order differs from the reference kernel (|d out| ~1e-6).
// ---------------------------------------------------------------------------------------------
constexpr int FA_QT = 32;    // queries per workgroup
constexpr int FA_KT = 64;    // cache rows per LDS tile
constexpr int FA_QPW = 8;    // queries per wave (4 waves)

template <int LPR>
__global__ __launch_bounds__(256) void attention_prefill_tiled_kernel(float* __restrict__ output, const float* __restrict__ Q,
                                                                     const uint16_t* __restrict__ kc, const uint16_t* __restrict__ vc,
                                                                     int T, int start_pos, int n_heads, int n_kv_heads, float scale) {
    constexpr int HD = 8 * LPR, PPW = 64 / LPR;
    extern __shared__ __attribute__((aligned(16))) uint8_t fa_lds[];
    uint16_t* kt = reinterpret_cast<uint16_t*>(fa_lds);                 // [FA_KT][HD] halves
    uint16_t* vt = kt + FA_KT * HD;                                     // [FA_KT][HD]
    float* qt = reinterpret_cast<float*>(vt + FA_KT * HD);              // [FA_QT][HD] queries of the tile
    const int head = blockIdx.x, q0 = blockIdx.y * FA_QT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int kv_head = head / (n_heads / n_kv_heads);
    const size_t stride = (size_t)n_kv_heads * HD;
    const int sub = lane / LPR, part_i = lane % LPR;
    const int nq = min(FA_QT, T - q0);                                  // queries in this tile
    for (int i = tid; i < nq * HD; i += 256) qt[i] = Q[((size_t)(q0 + i / HD) * n_heads + head) * HD + (i % HD)];
    float m[FA_QPW], l[FA_QPW], acc[FA_QPW][8];
#pragma unroll
    for (int u = 0; u < FA_QPW; ++u) {
        m[u] = -INFINITY; l[u] = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[u][j] = 0.0f;
    }
    const int n_keys = start_pos + q0 + nq;                             // keys 0 .. n_keys-1 are visible to the last query of the tile
    for (int k0 = 0; k0 < n_keys; k0 += FA_KT) {
        __syncthreads();                                                // the previous tile has been consumed (and qt is written)
        const int nk = min(FA_KT, n_keys - k0);
        for (int i = tid; i < nk * LPR; i += 256) {                     // 16-byte pieces, contiguous per cache row
            const int r = i / LPR, c = i % LPR;
            const size_t g = (size_t)(k0 + r) * stride + (size_t)kv_head * HD + 8 * c;
            *reinterpret_cast<u32x4*>(kt + r * HD + 8 * c) = *reinterpret_cast<const u32x4*>(kc + g);
            *reinterpret_cast<u32x4*>(vt + r * HD + 8 * c) = *reinterpret_cast<const u32x4*>(vc + g);
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < FA_QPW; ++u) {
            const int qi = wave * FA_QPW + u;                           // query of the tile (wave-uniform)
            if (qi >= nq) continue;
            const int last = start_pos + q0 + qi;                       // causal limit: keys <= last
            if (k0 > last) continue;
            float qreg[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) qreg[j] = qt[qi * HD + 8 * part_i + j];
            const int kend = min(nk, last - k0 + 1);
            for (int r0 = 0; r0 < kend; r0 += PPW) {
                const int r = r0 + sub, rr = min(r, kend - 1);          // past the causal limit: a valid row (finite values), weight 0
                float kf[8], vf[8];
                unpack8(*reinterpret_cast<const u32x4*>(kt + rr * HD + 8 * part_i), kf);
                unpack8(*reinterpret_cast<const u32x4*>(vt + rr * HD + 8 * part_i), vf);
                float sc = 0.0f;
#pragma unroll
                for (int j = 0; j < 8; ++j) sc = fmaf(qreg[j], kf[j], sc);
                sc = group_sum<LPR>(sc);
                sc = r < kend ? sc * scale : -INFINITY;
                const float mn = fmaxf(m[u], sc);
                const float a = (mn == -INFINITY) ? 1.0f : expf(m[u] - mn), pw = (mn == -INFINITY) ? 0.0f : expf(sc - mn);
                l[u] = fmaf(l[u], a, pw);
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[u][j] = fmaf(acc[u][j], a, pw * vf[j]);
                m[u] = mn;
            }
        }
    }
    // merge the PPW position groups of the wave per query, normalise, store
#pragma unroll
    for (int u = 0; u < FA_QPW; ++u) {
        const int qi = wave * FA_QPW + u;
        if (qi >= nq) continue;
        float mm = m[u], ll = l[u];
#pragma unroll
        for (int off = LPR; off < 64; off <<= 1) {
            const float mo = __shfl_xor(mm, off, 64), lo = __shfl_xor(ll, off, 64);
            const float mn = fmaxf(mm, mo);
            const float wa = (mm == -INFINITY) ? 0.0f : expf(mm - mn), wb = (mo == -INFINITY) ? 0.0f : expf(mo - mn);
            ll = fmaf(ll, wa, lo * wb);
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[u][j] = fmaf(acc[u][j], wa, __shfl_xor(acc[u][j], off, 64) * wb);
            mm = mn;
        }
        if (sub == 0) {
            const float inv = ll > 0.0f ? 1.0f / ll : 0.0f;             // reference attention.cu:293
            float* o = output + ((size_t)(q0 + qi) * n_heads + head) * HD + 8 * part_i;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = acc[u][j] * inv;
        }
    }
}

__global__ void rope_kernel(float* __restrict__ q, float* __restrict__ k, const int* __restrict__ positions, int seq_len,
                            int n_heads, int n_kv_heads, int head_dim, float theta, float fscale, int interleaved,
                            const float* __restrict__ inv_freq) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int half_dim = head_dim / 2;
    const int total_q = seq_len * n_heads * half_dim, total_k = seq_len * n_kv_heads * half_dim;
    if (idx >= total_q + total_k) return;
    const bool is_key = idx >= total_q;
    const int local = is_key ? idx - total_q : idx;
    const int n_h = is_key ? n_kv_heads : n_heads;
    const int pair = local % half_dim, head = (local / half_dim) % n_h, sp = local / (half_dim * n_h);
    float* data = (is_key ? k : q) + ((size_t)sp * n_h + head) * head_dim;
    const int i0 = interleaved ? 2 * pair : pair, i1 = interleaved ? 2 * pair + 1 : pair + half_dim;
    float a = data[i0], b = data[i1];
    rope_pair(a, b, positions[sp], pair, head_dim, theta, fscale, inv_freq);
    data[i0] = a;
    data[i1] = b;
}

// The same rotation for a prompt: one workgroup per token evaluates the token's head_dim / 2 (cos, sin) pairs ONCE -- the correctly
// rounded frequency, cosf, sinf of rope_pair(), bit for bit -- and applies them to all n_heads + n_kv_heads heads (rope_kernel
// re-evaluates pow / cosf / sinf for every head: 40 times per pair on the 8B shapes, 29 us per 1024-token layer against the ~8 us the
// 42 MB of traffic take).  head_dim <= 256.
__global__ __launch_bounds__(256) void rope_rows_kernel(float* __restrict__ q, float* __restrict__ k, const int* __restrict__ positions,
                                                        int n_heads, int n_kv_heads, int head_dim, float theta, float fscale, int interleaved,
                                                        const float* __restrict__ inv_freq) {
    __shared__ float cs[2][128];
    const int sp = blockIdx.x, half_dim = head_dim / 2;
    const int pos = positions[sp];
    for (int i = threadIdx.x; i < half_dim; i += blockDim.x) {
        const float freq = rope_freq(inv_freq, i, head_dim, theta);
        const float angle = pos * freq * fscale;
        cs[0][i] = cosf(angle);
        cs[1][i] = sinf(angle);
    }
    __syncthreads();
    const int total = (n_heads + n_kv_heads) * half_dim;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int pair = idx % half_dim, head = idx / half_dim;
        float* data = head < n_heads ? q + ((size_t)sp * n_heads + head) * head_dim : k + ((size_t)sp * n_kv_heads + (head - n_heads)) * head_dim;
        const int i0 = interleaved ? 2 * pair : pair, i1 = interleaved ? 2 * pair + 1 : pair + half_dim;
        const float a = data[i0], b = data[i1], c = cs[0][pair], sn = cs[1][pair];
        rope_rotate(a, b, c, sn, data[i0], data[i1]);
    }
}

// ... and the same launch also stores the token's K (rotated) and V rows into the half-precision caches (kv_store_kernel's conversions of the same
// values: identical cache rows); q is rotated in place, k and v are only read.  One launch instead of two per prompt layer.
// (the work of one workgroup = one token: q / k / v are the token's rows, pos its rotation position, cp its cache row -- shared by the segmented launch below)
__device__ __forceinline__ void rope_kv_store_row(float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v, const int pos,
                                                  const int n_heads, const int n_kv_heads, const int head_dim, const float theta, const float fscale,
                                                  const int interleaved, uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, const int cp,
                                                  const int max_seq, const float* __restrict__ inv_freq) {
    __shared__ float cs[2][128];
    const int half_dim = head_dim / 2;
    for (int i = threadIdx.x; i < half_dim; i += blockDim.x) {
        const float freq = rope_freq(inv_freq, i, head_dim, theta);
        const float angle = pos * freq * fscale;
        cs[0][i] = cosf(angle);
        cs[1][i] = sinf(angle);
    }
    __syncthreads();
    const int per_pos = n_kv_heads * head_dim;
    const bool store = cp < max_seq;   // reference attention.cu:336
    const int total = (n_heads + n_kv_heads) * half_dim;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int pair = idx % half_dim, head = idx / half_dim;
        const int i0 = interleaved ? 2 * pair : pair, i1 = interleaved ? 2 * pair + 1 : pair + half_dim;
        const float c = cs[0][pair], sn = cs[1][pair];
        if (head < n_heads) {
            float* data = q + (size_t)head * head_dim;
            const float a = data[i0], b = data[i1];
            rope_rotate(a, b, c, sn, data[i0], data[i1]);
        } else {
            const int kh = head - n_heads;
            const float* data = k + (size_t)kh * head_dim;
            float ra, rb;
            rope_rotate(data[i0], data[i1], c, sn, ra, rb);
            if (store) {
                uint16_t* row = kc + (size_t)cp * per_pos + (size_t)kh * head_dim;
                row[i0] = f2h(ra);
                row[i1] = f2h(rb);
            }
        }
    }
    if (store)
        for (int e = threadIdx.x; e < per_pos; e += blockDim.x) vc[(size_t)cp * per_pos + e] = f2h(v[e]);
}

__global__ __launch_bounds__(256) void rope_kv_store_rows_kernel(float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                 const int* __restrict__ positions, int n_heads, int n_kv_heads, int head_dim, float theta,
                                                                 float fscale, int interleaved, uint16_t* __restrict__ kc, uint16_t* __restrict__ vc,
                                                                 int start_pos, int max_seq, const float* __restrict__ inv_freq) {
    const int sp = blockIdx.x;
    rope_kv_store_row(q + (size_t)sp * n_heads * head_dim, k + (size_t)sp * n_kv_heads * head_dim, v + (size_t)sp * n_kv_heads * head_dim, positions[sp],
                      n_heads, n_kv_heads, head_dim, theta, fscale, interleaved, kc, vc, start_pos + sp, max_seq, inv_freq);
}

// ... for the rows of a PACKED pass (ntk_rope_kv_store_segments): row blockIdx.x belongs to the segment a uniform scan of the <= 16 row0 values finds; its
// position -- for the rotation and for the store -- is start_pos[s] + (row - row0[s]); its caches are segment s's.  The descriptor travels in the arguments.
struct RopeSegments {
    uint16_t* k[NTK_ATTN_BATCH_MAX];
    uint16_t* v[NTK_ATTN_BATCH_MAX];
    int row0[NTK_ATTN_BATCH_MAX], start_pos[NTK_ATTN_BATCH_MAX];
    int n_seg;
};
__global__ __launch_bounds__(256) void rope_kv_store_segments_kernel(float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                     const RopeSegments segs, int n_heads, int n_kv_heads, int head_dim, float theta,
                                                                     float fscale, int interleaved, int max_seq, const float* __restrict__ inv_freq) {
    const int row = blockIdx.x;
    int s = 0;
    while (s + 1 < segs.n_seg && row >= segs.row0[s + 1]) ++s;   // (uniform)
    const int pos = segs.start_pos[s] + (row - segs.row0[s]);
    rope_kv_store_row(q + (size_t)row * n_heads * head_dim, k + (size_t)row * n_kv_heads * head_dim, v + (size_t)row * n_kv_heads * head_dim, pos, n_heads,
                      n_kv_heads, head_dim, theta, fscale, interleaved, segs.k[s], segs.v[s], pos, max_seq, inv_freq);
}

__global__ void kv_store_kernel(uint16_t* __restrict__ kc, uint16_t* __restrict__ vc, const float* __restrict__ k,
                                const float* __restrict__ v, int total, int per_pos, int start_pos, int max_seq) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    const int t = idx / per_pos, e = idx % per_pos;
    const int cp = start_pos + t;
    if (cp >= max_seq) return;   // reference attention.cu:336
    kc[(size_t)cp * per_pos + e] = f2h(k[idx]);
    vc[(size_t)cp * per_pos + e] = f2h(v[idx]);
}

static size_t attn_lds(int hd, int n_keys, int nvec) {
    return sizeof(float) * ((size_t)nvec * hd + 16 + 4 * (size_t)hd + (size_t)n_keys + 1);
}

int launch_attention_decode_kvhead_mfma(float* part, const float* q, const float* k, const float* v, uint16_t* kc, uint16_t* vc,
                                        const int* d_pos, const float* inv_freq, int nh, int nkv, int max_seq, float scale, float theta,
                                        float fscale, int nsplit, float* merged_output, unsigned* counters, hipStream_t st);   // attention_mfma.hip
int launch_attention_prefill_mfma(float* out, const float* Q, const uint16_t* kc, const uint16_t* vc, int T, int start_pos, int nh, int nkv,
                                  int hd, float scale, hipStream_t st);   // attention_mfma.hip
int launch_attention_prefill_mfma_segments(float* out, const float* Q, const ntk_kv_segments& segs, const bool* mfma, int nh, int nkv, float scale,
                                           hipStream_t st);   // attention_mfma.hip

// (tuning builds only: the older prompt kernels)
static bool prefill_tiled_off() { static const bool off = NTK_TUNE_ENV_INT("NTK_PREFILL_ATTENTION_1TO1", 0) != 0; return off; }
static bool prefill_mfma_off() { static const bool off = NTK_TUNE_ENV_INT("NTK_PREFILL_ATTENTION_NO_MFMA", 0) != 0; return off; }

static int launch_attention(float* out, const float* Q, const void* kc, const void* vc, int T, int n_keys_base, int causal,
                            int nh, int nkv, int hd, float scale, hipStream_t st) {
    if (nh <= 0 || nkv <= 0 || hd <= 0 || nh % nkv != 0 || T < 0) return NTK_E_SHAPE;
    if (T == 0) return NTK_OK;
    const int max_keys = causal ? n_keys_base + T : n_keys_base;
    const bool aligned = (reinterpret_cast<uintptr_t>(kc) & 15) == 0 && (reinterpret_cast<uintptr_t>(vc) & 15) == 0;
    const uint16_t* k16 = static_cast<const uint16_t*>(kc);
    const uint16_t* v16 = static_cast<const uint16_t*>(vc);
    const bool tiled_off = prefill_tiled_off(), mfma_off = prefill_mfma_off();
    if (causal && T > 1 && aligned && hd == 128 && !tiled_off && !mfma_off) {   // prompt, head_dim 128: F16 matrix cores (attention_mfma.hip)
        const int rc = launch_attention_prefill_mfma(out, Q, k16, v16, T, n_keys_base, nh, nkv, hd, scale, st);
        if (rc != NTK_E_SHAPE && rc != NTK_E_ALIGN) return rc;
    }
    if (causal && T > 1 && aligned && (hd == 64 || hd == 128 || hd == 256) && !tiled_off) {   // prompt: flash-style tiles
        const size_t fl = (size_t)2 * FA_KT * hd * sizeof(uint16_t) + (size_t)FA_QT * hd * sizeof(float);
        const dim3 fgrid(nh, (T + FA_QT - 1) / FA_QT);
        if (hd == 128) hipLaunchKernelGGL(attention_prefill_tiled_kernel<16>, fgrid, dim3(256), fl, st, out, Q, k16, v16, T, n_keys_base, nh, nkv, scale);
        else if (hd == 64) hipLaunchKernelGGL(attention_prefill_tiled_kernel<8>, fgrid, dim3(256), fl, st, out, Q, k16, v16, T, n_keys_base, nh, nkv, scale);
        else {
            static bool once = hipFuncSetAttribute(reinterpret_cast<const void*>(attention_prefill_tiled_kernel<32>),
                                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)fl) == hipSuccess;
            if (!once) return NTK_E_LAUNCH;
            hipLaunchKernelGGL(attention_prefill_tiled_kernel<32>, fgrid, dim3(256), fl, st, out, Q, k16, v16, T, n_keys_base, nh, nkv, scale);
        }
        return last_launch_status();
    }
    const size_t lds = attn_lds(hd, max_keys, 1);
    if (lds > 160 * 1024) return NTK_E_SHAPE;
    dim3 grid(nh, T), block(256);
    // more than 64 KiB of dynamic LDS (contexts beyond ~15K keys) must be opted into per kernel
#define NTK_ATT(LPR_)                                                                                                   \
    do {                                                                                                                \
        if (lds > 64 * 1024)                                                                                            \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(attention_kernel<LPR_>),                            \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                            \
        hipLaunchKernelGGL(attention_kernel<LPR_>, grid, block, lds, st, out, Q, k16, v16, n_keys_base, causal, nh, nkv, hd, scale); \
    } while (0)
    if (aligned && hd == 128) NTK_ATT(16);
    else if (aligned && hd == 64) NTK_ATT(8);
    else if (aligned && hd == 256) NTK_ATT(32);
    else NTK_ATT(0);
#undef NTK_ATT
    return last_launch_status();
}

// the combine launch for partial states written by another translation unit (attention_q8.hip)
int launch_attention_split_combine(float* output, const float* part, int n_heads, int hd, int nsplit, int n_kv_heads, hipStream_t st) {
    hipLaunchKernelGGL(attention_split_combine_kernel, dim3(n_heads), dim3(128), 0, st, output, part, hd, nsplit, n_kv_heads);
    return last_launch_status();
}

}  // namespace ntk

extern "C" {

// The prompt-side rotations with the per-pair frequencies from a DEVICE table (inv_freq [head_dim / 2]: entry i replaces the in-kernel 1 / pow(theta,
// 2i / head_dim); NULL: the in-kernel frequency, which is what the entry points without _tab pass)
int ntk_rope_tab(float* q, float* k, const int* positions, int /*batch_size*/, int seq_len, int n_heads, int n_kv_heads,
                 int head_dim, float theta_base, float freq_scale, int interleaved, const float* inv_freq, void* stream) {
    if (!q || !k || !positions) return NTK_E_NULL;
    if (seq_len < 0 || n_heads < 0 || n_kv_heads < 0 || head_dim <= 0 || (head_dim & 1)) return NTK_E_SHAPE;
    const int total = seq_len * (n_heads + n_kv_heads) * (head_dim / 2);
    if (total == 0) return NTK_OK;
    if (seq_len >= 4 && head_dim <= 256)   // prompts: the token's (cos, sin) pairs once for all heads
        hipLaunchKernelGGL(ntk::rope_rows_kernel, dim3(seq_len), dim3(256), 0, ntk::resolve_stream(stream), q, k, positions, n_heads, n_kv_heads,
                           head_dim, theta_base, freq_scale, interleaved, inv_freq);
    else
        hipLaunchKernelGGL(ntk::rope_kernel, dim3((total + 255) / 256), dim3(256), 0, ntk::resolve_stream(stream), q, k,
                           positions, seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale, interleaved, inv_freq);
    return ntk::last_launch_status();
}

int ntk_rope(float* q, float* k, const int* positions, int batch_size, int seq_len, int n_heads, int n_kv_heads,
             int head_dim, float theta_base, float freq_scale, int interleaved, void* stream) {
    return ntk_rope_tab(q, k, positions, batch_size, seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale, interleaved, nullptr, stream);
}

int ntk_rope_kv_store_tab(float* q, const float* k, const float* v, const int* positions, int seq_len, int n_heads, int n_kv_heads, int head_dim,
                          float theta_base, float freq_scale, int interleaved, void* k_cache, void* v_cache, int start_pos, int max_seq,
                          const float* inv_freq, void* stream) {
    if (!q || !k || !v || !positions || !k_cache || !v_cache) return NTK_E_NULL;
    if (seq_len < 0 || n_heads <= 0 || n_kv_heads <= 0 || head_dim <= 0 || (head_dim & 1) || head_dim > 256 || start_pos < 0 || max_seq <= 0) return NTK_E_SHAPE;
    if (seq_len == 0) return NTK_OK;
    hipLaunchKernelGGL(ntk::rope_kv_store_rows_kernel, dim3(seq_len), dim3(256), 0, ntk::resolve_stream(stream), q, k, v, positions, n_heads, n_kv_heads,
                       head_dim, theta_base, freq_scale, interleaved, static_cast<uint16_t*>(k_cache), static_cast<uint16_t*>(v_cache), start_pos, max_seq,
                       inv_freq);
    return ntk::last_launch_status();
}

int ntk_rope_kv_store(float* q, const float* k, const float* v, const int* positions, int seq_len, int n_heads, int n_kv_heads, int head_dim,
                      float theta_base, float freq_scale, int interleaved, void* k_cache, void* v_cache, int start_pos, int max_seq, void* stream) {
    return ntk_rope_kv_store_tab(q, k, v, positions, seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale, interleaved, k_cache, v_cache, start_pos,
                                 max_seq, nullptr, stream);
}

int ntk_copy_to_kv_cache(void* k_cache, void* v_cache, const float* k, const float* v, int seq_len, int n_kv_heads,
                         int head_dim, int start_pos, int max_seq, void* stream) {
    if (!k_cache || !v_cache || !k || !v) return NTK_E_NULL;
    if (seq_len < 0 || n_kv_heads <= 0 || head_dim <= 0 || start_pos < 0) return NTK_E_SHAPE;
    const int per = n_kv_heads * head_dim, total = seq_len * per;
    if (total == 0) return NTK_OK;
    hipLaunchKernelGGL(ntk::kv_store_kernel, dim3((total + 255) / 256), dim3(256), 0, ntk::resolve_stream(stream),
                       static_cast<uint16_t*>(k_cache), static_cast<uint16_t*>(v_cache), k, v, total, per, start_pos, max_seq);
    return ntk::last_launch_status();
}

int ntk_attention_decode(float* output, const float* q, const void* k_cache, const void* v_cache, int seq_len, int n_heads,
                         int n_kv_heads, int head_dim, int /*max_seq*/, float scale, void* stream) {
    if (!output || !q || !k_cache || !v_cache) return NTK_E_NULL;
    if (seq_len <= 0) return NTK_E_SHAPE;
    return ntk::launch_attention(output, q, k_cache, v_cache, 1, seq_len, 0, n_heads, n_kv_heads, head_dim, scale,
                                 ntk::resolve_stream(stream));
}

int ntk_attention_prefill(float* output, const float* Q, const void* k_cache, const void* v_cache, int seq_len, int start_pos,
                          int n_heads, int n_kv_heads, int head_dim, int /*max_seq*/, float scale, void* stream) {
    if (!output || !Q || !k_cache || !v_cache) return NTK_E_NULL;
    if (seq_len < 0 || start_pos < 0) return NTK_E_SHAPE;
    return ntk::launch_attention(output, Q, k_cache, v_cache, seq_len, start_pos, 1, n_heads, n_kv_heads, head_dim, scale,
                                 ntk::resolve_stream(stream));
}

// the descriptor of a packed pass (ntk_engine.h); total_rows < 0: whatever its segments sum to
static int kv_segments_check(const ntk_kv_segments* segs, int total_rows, int max_seq) {
    if (!segs) return NTK_E_NULL;
    if (segs->n_seg < 1 || segs->n_seg > NTK_ATTN_BATCH_MAX || max_seq <= 0) return NTK_E_SHAPE;
    long long rows = 0;
    for (int s = 0; s < segs->n_seg; ++s) {
        if (segs->row0[s] != rows || segs->n_rows[s] < 1 || segs->start_pos[s] < 0) return NTK_E_SHAPE;
        if ((long long)segs->start_pos[s] + segs->n_rows[s] > max_seq) return NTK_E_SHAPE;
        rows += segs->n_rows[s];
    }
    if (rows > 0x7FFFFFFF || (total_rows >= 0 && rows != total_rows)) return NTK_E_SHAPE;
    for (int s = 0; s < segs->n_seg; ++s) {
        if (!segs->k[s] || !segs->v[s]) return NTK_E_NULL;
        for (int t = 0; t < s; ++t)
            if (segs->k[t] == segs->k[s]) return NTK_E_SHAPE;   // two segments of one pass would write (and attend over) the same cache
    }
    return NTK_OK;
}

int ntk_kv_segments_validate(const ntk_kv_segments* segs, int total_rows, int max_seq) {
    if (total_rows < 0) return segs ? NTK_E_SHAPE : NTK_E_NULL;
    return kv_segments_check(segs, total_rows, max_seq);
}

int ntk_rope_kv_store_segments_tab(float* q, const float* k, const float* v, const ntk_kv_segments* segs, int n_heads, int n_kv_heads, int head_dim,
                                   float theta_base, float freq_scale, int interleaved, int max_seq, const float* inv_freq, void* stream) {
    if (!q || !k || !v || !segs) return NTK_E_NULL;
    if (n_heads <= 0 || n_kv_heads <= 0 || head_dim <= 0 || (head_dim & 1) || head_dim > 256) return NTK_E_SHAPE;
    const int rc = kv_segments_check(segs, -1, max_seq);
    if (rc != NTK_OK) return rc;
    ntk::RopeSegments d{};
    for (int s = 0; s < NTK_ATTN_BATCH_MAX; ++s) {   // (entries past n_seg: never indexed, the scan stops at n_seg - 1)
        const int u = s < segs->n_seg ? s : 0;
        d.k[s] = static_cast<uint16_t*>(segs->k[u]); d.v[s] = static_cast<uint16_t*>(segs->v[u]);
        d.row0[s] = segs->row0[u]; d.start_pos[s] = segs->start_pos[u];
    }
    d.n_seg = segs->n_seg;
    const int rows = segs->row0[segs->n_seg - 1] + segs->n_rows[segs->n_seg - 1];
    hipLaunchKernelGGL(ntk::rope_kv_store_segments_kernel, dim3(rows), dim3(256), 0, ntk::resolve_stream(stream), q, k, v, d, n_heads, n_kv_heads, head_dim,
                       theta_base, freq_scale, interleaved, max_seq, inv_freq);
    return ntk::last_launch_status();
}

int ntk_rope_kv_store_segments(float* q, const float* k, const float* v, const ntk_kv_segments* segs, int n_heads, int n_kv_heads, int head_dim,
                               float theta_base, float freq_scale, int interleaved, int max_seq, void* stream) {
    return ntk_rope_kv_store_segments_tab(q, k, v, segs, n_heads, n_kv_heads, head_dim, theta_base, freq_scale, interleaved, max_seq, nullptr, stream);
}

int ntk_attention_prefill_segments(float* output, const float* Q, const ntk_kv_segments* segs, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                                   float scale, void* stream) {
    if (!output || !Q || !segs) return NTK_E_NULL;
    if (n_heads <= 0 || n_kv_heads <= 0 || head_dim <= 0 || n_heads % n_kv_heads != 0) return NTK_E_SHAPE;
    int rc = kv_segments_check(segs, -1, max_seq);
    if (rc != NTK_OK) return rc;
    hipStream_t st = ntk::resolve_stream(stream);
    // which segments ntk_attention_prefill would hand to the matrix-core kernel (launch_attention's rule + launch_attention_prefill_mfma's alignment
    // check; a segment's rows of Q / output start a multiple of 512 bytes behind the arrays' first): those share ONE launch of that kernel's body
    const bool io_aligned = (reinterpret_cast<uintptr_t>(Q) & 15) == 0 && (reinterpret_cast<uintptr_t>(output) & 15) == 0;
    bool mfma[NTK_ATTN_BATCH_MAX] = {};
    bool any = false;
    for (int s = 0; s < segs->n_seg; ++s) {
        const bool aligned = (reinterpret_cast<uintptr_t>(segs->k[s]) & 15) == 0 && (reinterpret_cast<uintptr_t>(segs->v[s]) & 15) == 0;
        mfma[s] = segs->n_rows[s] > 1 && aligned && io_aligned && head_dim == 128 && !ntk::prefill_tiled_off() && !ntk::prefill_mfma_off();
        any = any || mfma[s];
    }
    if (any) {
        rc = ntk::launch_attention_prefill_mfma_segments(output, Q, *segs, mfma, n_heads, n_kv_heads, scale, st);
        if (rc != NTK_OK) return rc;
    }
    // the single-row segments with 16-byte aligned caches at head_dim 64 / 128 / 256: ONE launch of the single-query kernel's body, which is what
    // ntk_attention_prefill runs for a one-row prompt
    ntk::SingleRows one{};
    int n_one = 0, max_keys = 0;
    bool single[NTK_ATTN_BATCH_MAX] = {};
    for (int s = 0; s < segs->n_seg && (head_dim == 64 || head_dim == 128 || head_dim == 256); ++s) {
        const bool aligned = (reinterpret_cast<uintptr_t>(segs->k[s]) & 15) == 0 && (reinterpret_cast<uintptr_t>(segs->v[s]) & 15) == 0;
        if (segs->n_rows[s] != 1 || !aligned) continue;
        single[s] = true;
        one.k[n_one] = static_cast<const uint16_t*>(segs->k[s]); one.v[n_one] = static_cast<const uint16_t*>(segs->v[s]);
        one.row0[n_one] = segs->row0[s]; one.start_pos[n_one] = segs->start_pos[s];
        max_keys = segs->start_pos[s] + 1 > max_keys ? segs->start_pos[s] + 1 : max_keys;
        ++n_one;
    }
    if (n_one > 0) {
        const size_t lds = ntk::attn_lds(head_dim, max_keys, 1);   // (the score row of the longest prefix: a larger allocation changes no result)
        if (lds > 160 * 1024) return NTK_E_SHAPE;
#define NTK_ATT1(LPR_)                                                                                                          \
    do {                                                                                                                        \
        if (lds > 64 * 1024)                                                                                                    \
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ntk::attention_single_rows_kernel<LPR_>),                   \
                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                                    \
        hipLaunchKernelGGL(ntk::attention_single_rows_kernel<LPR_>, dim3(n_heads, n_one), dim3(256), lds, st, output, Q, one, n_heads, n_kv_heads, \
                           head_dim, scale);                                                                                    \
    } while (0)
        if (head_dim == 128) NTK_ATT1(16);
        else if (head_dim == 64) NTK_ATT1(8);
        else NTK_ATT1(32);
#undef NTK_ATT1
        rc = ntk::last_launch_status();
        if (rc != NTK_OK) return rc;
    }
    // every other segment: ntk_attention_prefill's own launch on the segment alone (head_dim 64 / 256: the tiled kernel; unaligned caches, other head sizes)
    for (int s = 0; s < segs->n_seg; ++s) {
        if (mfma[s] || single[s]) continue;
        const size_t row = (size_t)segs->row0[s] * n_heads * head_dim;
        rc = ntk::launch_attention(output + row, Q + row, segs->k[s], segs->v[s], segs->n_rows[s], segs->start_pos[s], 1, n_heads, n_kv_heads, head_dim, scale, st);
        if (rc != NTK_OK) return rc;
    }
    return NTK_OK;
}

int ntk_attention_decode_fused(float* output, const float* q, const float* k, const float* v, void* k_cache, void* v_cache,
                               const int* d_pos, const float* inv_freq, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                               float scale, float theta_base, float freq_scale, void* stream) {
    if (!output || !q || !k || !v || !k_cache || !v_cache || !d_pos) return NTK_E_NULL;
    if (n_heads <= 0 || n_kv_heads <= 0 || n_heads % n_kv_heads != 0 || head_dim <= 0 || (head_dim & 1) || max_seq <= 0)
        return NTK_E_SHAPE;
    if ((size_t)max_seq * n_kv_heads * head_dim * 2 >= 0xF0000000ull) return NTK_E_SHAPE;   // (32-bit row offsets inside one layer's cache)
    hipStream_t st = ntk::resolve_stream(stream);
    const bool aligned = (reinterpret_cast<uintptr_t>(k_cache) & 15) == 0 && (reinterpret_cast<uintptr_t>(v_cache) & 15) == 0;
    uint16_t* k16 = static_cast<uint16_t*>(k_cache);
    uint16_t* v16 = static_cast<uint16_t*>(v_cache);
    if (aligned && (head_dim == 128 || head_dim == 64 || head_dim == 256)) {   // single-pass kernel
        const int G = 4 * (64 / (head_dim / 8));
        const size_t lds = sizeof(float) * ((size_t)3 * head_dim + 2 * G + (size_t)G * head_dim);
#define NTK_ATTV(...) hipLaunchKernelGGL((ntk::attention_decode_fused_v3_kernel<__VA_ARGS__>), dim3(n_heads), dim3(256), lds, st, output, q, k, v, \
                                           k16, v16, d_pos, inv_freq, n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base, freq_scale)
        if (head_dim == 128) NTK_ATTV(16, 4);
        else if (head_dim == 64) NTK_ATTV(8, 4);
        else NTK_ATTV(32, 4);
#undef NTK_ATTV
        return ntk::last_launch_status();
    }
    const size_t lds = ntk::attn_lds(head_dim, max_seq, 3);
    if (lds > 160 * 1024) return NTK_E_SHAPE;
    if (lds > 64 * 1024)
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ntk::attention_decode_fused_kernel<0>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(ntk::attention_decode_fused_kernel<0>, dim3(n_heads), dim3(256), lds, st, output, q, k, v, k16, v16, d_pos,
                       n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base, freq_scale);
    return ntk::last_launch_status();
}

size_t ntk_attention_split_scratch_bytes(int n_heads, int head_dim, int nsplit) {
    return ntk::att_merge_header_bytes(n_heads) + (size_t)n_heads * (size_t)nsplit * (size_t)(head_dim + 2) * sizeof(float);
}

int ntk_attention_split_scratch_init(float* scratch, int n_heads, void* stream) {
    if (!scratch) return NTK_E_NULL;
    if (n_heads <= 0) return NTK_E_SHAPE;
    return hipMemsetAsync(scratch, 0, ntk::att_merge_header_bytes(n_heads), ntk::resolve_stream(stream)) == hipSuccess ? NTK_OK : NTK_E_LAUNCH;
}

static int attention_decode_split_impl(float* output, const float* q, const float* k, const float* v, void* k_cache, void* v_cache,
                                       const int* d_pos, const float* inv_freq, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                                       float scale, float theta_base, float freq_scale, int nsplit, float* scratch_all, void* stream, bool merged) {
    if (!output || !q || !k || !v || !k_cache || !v_cache || !d_pos || !scratch_all) return NTK_E_NULL;
    if (n_heads <= 0 || n_kv_heads <= 0 || n_heads % n_kv_heads != 0 || max_seq <= 0 || nsplit < 1 || nsplit > 1024)
        return NTK_E_SHAPE;
    if (merged && nsplit > ntk::ATT_MERGE_MAX_SPLITS) return NTK_E_SHAPE;
    unsigned* counters = reinterpret_cast<unsigned*>(scratch_all);   // (zero outside the merged launches)
    float* scratch = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(scratch_all) + ntk::att_merge_header_bytes(n_heads));
    if (head_dim != 128 && head_dim != 64 && head_dim != 256) return NTK_E_SHAPE;   // 16-byte row pieces: the engine falls back to the single pass otherwise
    if ((size_t)max_seq * n_kv_heads * head_dim * 2 >= 0xF0000000ull) return NTK_E_SHAPE;   // (32-bit row offsets inside one layer's cache)
    if ((reinterpret_cast<uintptr_t>(k_cache) & 15) || (reinterpret_cast<uintptr_t>(v_cache) & 15)) return NTK_E_ALIGN;
    hipStream_t st = ntk::resolve_stream(stream);
    uint16_t* k16 = static_cast<uint16_t*>(k_cache);
    uint16_t* v16 = static_cast<uint16_t*>(v_cache);
    // head_dim 128, at most 16 query heads per KV head, 16 splits or more: the matrix-core form, one workgroup per (KV head, split), every
    // cache row read once (attention_mfma.hip).  With fewer splits a wave of that form walks four or more 32-row chunks per 4096 positions
    // and the per-query-head walk below is faster (measured, tools/attn_bench.py over 40 rotating layer caches, 8B geometry, us per layer
    // incl. the combine launch: 1023 positions 8.7 (walk, 8 splits) vs 10.2 (matrix cores, 8) -- 2047: 10.1 vs 11.1 (16) -- 4095: 13.5 vs
    // 12.75 (32); 70B geometry 4095: 16.5 vs 13.5; inside the engine the forms tie between 2300 and 3300 positions: profiles/r04_attention_kvhead_form.txt)
    static const int kvhead_form = NTK_TUNE_ENV_INT("NTK_ATTN_KVHEAD", 1);   // (tuning builds: 0 = the per-query-head walk, 2 = the matrix-core form at any split count)
    if (head_dim == 128 && n_heads / n_kv_heads <= 16 && ((kvhead_form == 1 && nsplit >= 16) || kvhead_form == 2)) {
        const int rc = ntk::launch_attention_decode_kvhead_mfma(scratch, q, k, v, k16, v16, d_pos, inv_freq, n_heads, n_kv_heads, max_seq,
                                                                scale, theta_base, freq_scale, nsplit, merged ? output : nullptr, counters, st);
        if (rc != NTK_OK || merged) return rc;
        hipLaunchKernelGGL(ntk::attention_split_combine_kernel, dim3(n_heads), dim3(128), 0, st, output, scratch, head_dim, nsplit, n_kv_heads);
        return ntk::last_launch_status();
    }
    const int G = 4 * (64 / (head_dim / 8));
    const size_t lds = sizeof(float) * ((size_t)3 * head_dim + 2 * G + (size_t)G * head_dim);
#define NTK_ATTSP(...) hipLaunchKernelGGL((ntk::attention_decode_split_kernel<__VA_ARGS__>), dim3(n_heads, nsplit), dim3(256), lds, st, scratch, q, k, \
                                           v, k16, v16, d_pos, inv_freq, n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base, freq_scale, output, counters)
    static const int split_d = NTK_TUNE_ENV_INT("NTK_ATTN_SPLIT_D", 4);   // (tuning builds: rows in flight per position group)
    if (merged) {
        if (head_dim == 128) NTK_ATTSP(16, 4, true);
        else if (head_dim == 64) NTK_ATTSP(8, 4, true);
        else NTK_ATTSP(32, 4, true);
        return ntk::last_launch_status();
    }
    if (head_dim == 128 && split_d == 8) NTK_ATTSP(16, 8, false);
    else if (head_dim == 128) NTK_ATTSP(16, 4, false);
    else if (head_dim == 64) NTK_ATTSP(8, 4, false);
    else NTK_ATTSP(32, 4, false);
#undef NTK_ATTSP
    if (ntk::last_launch_status() != NTK_OK) return NTK_E_LAUNCH;
    hipLaunchKernelGGL(ntk::attention_split_combine_kernel, dim3(n_heads), dim3(128), 0, st, output, scratch, head_dim, nsplit, n_kv_heads);
    return ntk::last_launch_status();
}

int ntk_attention_decode_split(float* output, const float* q, const float* k, const float* v, void* k_cache, void* v_cache,
                               const int* d_pos, const float* inv_freq, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                               float scale, float theta_base, float freq_scale, int nsplit, float* scratch, void* stream) {
    return attention_decode_split_impl(output, q, k, v, k_cache, v_cache, d_pos, inv_freq, n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base,
                                       freq_scale, nsplit, scratch, stream, false);
}

int ntk_attention_decode_split_merged(float* output, const float* q, const float* k, const float* v, void* k_cache, void* v_cache,
                                      const int* d_pos, const float* inv_freq, int n_heads, int n_kv_heads, int head_dim, int max_seq,
                                      float scale, float theta_base, float freq_scale, int nsplit, float* scratch, void* stream) {
    return attention_decode_split_impl(output, q, k, v, k_cache, v_cache, d_pos, inv_freq, n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base,
                                       freq_scale, nsplit, scratch, stream, true);
}

}  // extern "C"
