// moe.hip -- the routed expert FFN of mixture-of-experts models (GGUF blk.N.ffn_gate_inp.weight + ffn_{gate,up,down}_exps.weight: Qwen3-MoE, Mixtral).
// No reference counterpart: the reference runs dense Llama layers only.  Three entry points, each reading everything about the routing from DEVICE memory,
// so no launch parameter depends on which experts a token chose and the captured decode token stays a plain chain of nodes:
//
//   ntk_moe_route    logits = router . xn per row (F32), the K largest in descending order (ties: the lower expert), w = softmax over those K, and the
//                    expert-major work list: offsets[E + 1] and pairs[T K] = the pair indices t K + k sorted by (expert, pair index).  Two kernels: one
//                    workgroup per row, then ONE workgroup that counts and places (every expert's thread walks ids in ascending pair order: a stable
//                    counting sort without atomics, the same list on every launch).
//   ntk_moe_gate_up  act[p] = SiLU(Wg[e] . xn[t]) x (Wu[e] . xn[t]) for every pair p = t K + k, e = ids[p].  Grid (row block, expert): a workgroup whose
//                    expert has no pair exits at once.
//   ntk_moe_down     y[t] = resid[t] + sum_k w[t][k] (Wd[e_k] . act[t K + k]).  A workgroup OWNS a block of output rows: it walks the experts that have
//                    pairs, leaves every pair's products in `part`, and then sums its own rows over k in ascending order -- one thread per output element,
//                    no atomics, nothing crosses a workgroup.
//
// The GEMV both share (moe_row_dots): a WAVE takes one weight row of one expert, copies its GGUF bytes ONCE into a wave-private LDS image (16-byte pieces
// where the row's address allows, 2-byte pieces at its ends: Q6_K rows of 630 bytes start on every even address), and applies it to the expert's pairs
// kPairs at a time, x from L2.  Lane l decodes the 32-column units l, l + 64, ... (a Q8_0 block, a K-quant sub-block) and runs ONE chain of FMAs per pair
// over them in ascending column order; wave_sum ends it.  A short last chunk repeats its last pair, so the instructions a pair goes through -- and its
// bits -- do not depend on how many pairs share the row with it, on the chunk it falls into, or on T.
#include "common.hip.h"

namespace ntk {

typedef uint32_t moe_u32x4 __attribute__((ext_vector_type(4)));

constexpr int kMoeMaxE = 256, kMoeMaxK = 16, kMoeMaxT = 1024;
constexpr int kPairs = 4;        // pairs per pass over a staged row
constexpr int kMoeWaves = 4;     // waves per workgroup of the two GEMV kernels
constexpr size_t kMoeLdsMax = NTK_MOE_LDS_MAX;

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
// NP = kPairs, or 1 for a lone pair (a decode token: every active expert has one): the same chain per pair, so the same bits, without the discarded copies
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

// the pairs [beg, end) of expert e in the work list, held to the list's bounds whatever the buffer holds
__device__ __forceinline__ void moe_expert_range(const int* offsets, int e, int n_pairs, int& beg, int& end) {
    beg = offsets[e]; end = offsets[e + 1];
    if (beg < 0) beg = 0;
    if (end > n_pairs) end = n_pairs;
}

// ---- routing ---------------------------------------------------------------------------------------------------------------------------------------
struct MoeRouteArgs {
    const float* xn; const float* router;
    int* ids; float* w; float* logits;
    int hidden, E, K, vec;
};

// grid T, 256 threads: wave g takes experts g, g + 4, ...; wave 0 then selects
__global__ __launch_bounds__(256) void moe_route_rows_kernel(const MoeRouteArgs a) {
    __shared__ float s_logit[kMoeMaxE];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t = blockIdx.x;
    const float* const x = a.xn + (size_t)t * a.hidden;
    for (int e = wave; e < a.E; e += 4) {
        const float* const r = a.router + (size_t)e * a.hidden;
        float s = 0.0f;
        if (a.vec) {
            for (int i = lane; i < a.hidden / 4; i += 64) {
                const float4 xv = reinterpret_cast<const float4*>(x)[i], rv = reinterpret_cast<const float4*>(r)[i];
                s = fmaf(rv.x, xv.x, s); s = fmaf(rv.y, xv.y, s); s = fmaf(rv.z, xv.z, s); s = fmaf(rv.w, xv.w, s);
            }
        } else {
            for (int i = lane; i < a.hidden; i += 64) s = fmaf(r[i], x[i], s);
        }
        s = wave_sum(s);
        if (lane == 0) {
            s_logit[e] = s;
            if (a.logits) a.logits[(size_t)t * a.E + e] = s;
        }
    }
    __syncthreads();
    if (wave != 0) return;
    // lane l holds experts l, l + 64, l + 128, l + 192; K rounds of (largest value, lowest index) over the entries not yet taken
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int e = lane + 64 * j;
        const float f = e < a.E ? s_logit[e] : -INFINITY;
        v[j] = f == f ? f : -INFINITY;   // (a NaN logit ranks last instead of poisoning the comparisons)
    }
    unsigned taken = 0;
    float sel[kMoeMaxK];
    int sel_id[kMoeMaxK];
#pragma unroll
    for (int k = 0; k < kMoeMaxK; ++k) { sel[k] = 0.0f; sel_id[k] = 0; }
    for (int k = 0; k < a.K; ++k) {
        float bv = -INFINITY;
        int bi = 0x7FFFFFFF;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = lane + 64 * j;
            if (e < a.E && !((taken >> j) & 1u) && (bi == 0x7FFFFFFF || v[j] > bv)) { bv = v[j]; bi = e; }
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
    if (lane == 0) {   // softmax over the K selected logits: the largest comes first
        float ex[kMoeMaxK], sum = 0.0f;
#pragma unroll
        for (int k = 0; k < kMoeMaxK; ++k) {
            ex[k] = k < a.K ? expf(sel[k] - sel[0]) : 0.0f;
            if (k < a.K) sum += ex[k];
        }
#pragma unroll
        for (int k = 0; k < kMoeMaxK; ++k)
            if (k < a.K) {
                a.ids[(size_t)t * a.K + k] = sel_id[k];
                a.w[(size_t)t * a.K + k] = ex[k] / sum;
            }
    }
}

// ONE workgroup of 256 threads: thread e counts expert e's pairs, thread 0 lays the offsets out, thread e places its pairs in ascending pair order
__global__ __launch_bounds__(256) void moe_route_list_kernel(const int* __restrict__ ids, int* __restrict__ offsets, int* __restrict__ pairs, int n_pairs, int E) {
    __shared__ int s_count[kMoeMaxE], s_off[kMoeMaxE + 1];
    const int e = threadIdx.x;
    int c = 0;
    if (e < E) for (int p = 0; p < n_pairs; ++p) c += ids[p] == e ? 1 : 0;
    s_count[e] = e < E ? c : 0;
    __syncthreads();
    if (e == 0) {
        int run = 0;
        for (int i = 0; i < E; ++i) { s_off[i] = run; run += s_count[i]; }
        s_off[E] = run;
    }
    __syncthreads();
    if (e == 0) offsets[E] = s_off[E];   // (E may be 256: there is no thread 256)
    if (e < E) {
        offsets[e] = s_off[e];
        int at = s_off[e];
        for (int p = 0; p < n_pairs; ++p) if (ids[p] == e) pairs[at++] = p;
    }
}

// ---- gate | up -------------------------------------------------------------------------------------------------------------------------------------
struct MoeGateUpArgs {
    const uint8_t* wg; const uint8_t* wu;
    const float* xn; const int* offsets; const int* pairs;
    float* act;
    int dt_g, dt_u;
    unsigned rb_g, rb_u, img_g, img_u;   // row bytes and LDS image bytes
    int hidden, inter, E, K, n_pairs, rows_per_wg;
};

// one staged row pair against pairs [c0, c0 + NP) of the expert's list
template <int NP>
__device__ __forceinline__ void moe_gate_up_chunk(const MoeGateUpArgs& a, const uint8_t* st_g, const uint8_t* st_u, int og, int ou, int n_units, int lane, int row,
                                                  int c0, int end) {
    int p[NP];
    const float* x[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int at = c0 + j < end ? c0 + j : end - 1;   // a short last chunk repeats its last pair
        int pj = a.pairs[at];
        if (pj < 0 || pj >= a.n_pairs) pj = -1;            // (a list that is not ours: nothing is read or written for it)
        p[j] = c0 + j < end ? pj : -1;
        x[j] = a.xn + (size_t)((pj < 0 ? 0 : pj) / a.K) * a.hidden;
    }
    float g[NP], u[NP];
    moe_row_dots<NP>(g, a.dt_g, st_g, og, n_units, lane, x);
    moe_row_dots<NP>(u, a.dt_u, st_u, ou, n_units, lane, x);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NP; ++j)
            if (p[j] >= 0) a.act[(size_t)p[j] * a.inter + row] = g[j] / (1.0f + expf(-g[j])) * u[j];
    }
}

// grid (ceil(inter / rows_per_wg), E), 256 threads: wave g takes rows g, g + 4, ... of the block
__global__ __launch_bounds__(64 * kMoeWaves) void moe_gate_up_kernel(const MoeGateUpArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t moe_lds[];
    const int e = blockIdx.y;
    int beg, end;
    moe_expert_range(a.offsets, e, a.n_pairs, beg, end);
    if (end <= beg) return;   // nobody chose this expert
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint8_t* const st_g = moe_lds + (size_t)wave * (a.img_g + a.img_u);
    uint8_t* const st_u = st_g + a.img_g;
    const int row0 = blockIdx.x * a.rows_per_wg, n_units = a.hidden / 32;
    const uint8_t* const base_g = a.wg + (size_t)e * (size_t)a.inter * a.rb_g;
    const uint8_t* const base_u = a.wu + (size_t)e * (size_t)a.inter * a.rb_u;
    for (int r0 = 0; r0 < a.rows_per_wg; r0 += kMoeWaves) {   // (the same trip count in every wave: the barriers are the workgroup's)
        const int row = row0 + r0 + wave;
        const bool live = r0 + wave < a.rows_per_wg && row < a.inter;
        int og = 0, ou = 0;
        if (live) {
            og = moe_stage_row(st_g, base_g + (size_t)row * a.rb_g, a.rb_g, lane);
            ou = moe_stage_row(st_u, base_u + (size_t)row * a.rb_u, a.rb_u, lane);
        }
        __syncthreads();
        if (live) {
            for (int c0 = beg; c0 < end;) {   // four pairs at a time; a lone (last) pair alone
                if (end - c0 == 1) { moe_gate_up_chunk<1>(a, st_g, st_u, og, ou, n_units, lane, row, c0, end); c0 += 1; }
                else { moe_gate_up_chunk<kPairs>(a, st_g, st_u, og, ou, n_units, lane, row, c0, end); c0 += kPairs; }
            }
        }
        __syncthreads();
    }
}

// ---- down ------------------------------------------------------------------------------------------------------------------------------------------
struct MoeDownArgs {
    const uint8_t* wd;
    const float* act; const int* ids; const float* w; const int* offsets; const int* pairs;
    const float* resid; float* y; float* part;
    int dt;
    unsigned rb, img;
    int hidden, inter, E, K, T, n_pairs, rows_per_wg;
};

template <int NP>
__device__ __forceinline__ void moe_down_chunk(const MoeDownArgs& a, const uint8_t* st, int o, int n_units, int lane, int row, int c0, int end) {
    int p[NP];
    const float* x[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        const int at = c0 + j < end ? c0 + j : end - 1;
        int pj = a.pairs[at];
        if (pj < 0 || pj >= a.n_pairs) pj = -1;
        p[j] = c0 + j < end ? pj : -1;
        x[j] = a.act + (size_t)(pj < 0 ? 0 : pj) * a.inter;
    }
    float d[NP];
    moe_row_dots<NP>(d, a.dt, st, o, n_units, lane, x);
    if (lane == 0) {
#pragma unroll
        for (int j = 0; j < NP; ++j)
            if (p[j] >= 0) a.part[(size_t)p[j] * a.hidden + row] = d[j];
    }
}

// grid ceil(hidden / rows_per_wg), 256 threads: the workgroup owns output rows [row0, row0 + rows_per_wg)
__global__ __launch_bounds__(64 * kMoeWaves) void moe_down_kernel(const MoeDownArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t moe_lds[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint8_t* const st = moe_lds + (size_t)wave * a.img;
    const int row0 = blockIdx.x * a.rows_per_wg, n_units = a.inter / 32;
    for (int e = 0; e < a.E; ++e) {
        int beg, end;
        moe_expert_range(a.offsets, e, a.n_pairs, beg, end);
        if (end <= beg) continue;   // (the same for every wave of the workgroup)
        const uint8_t* const base = a.wd + (size_t)e * (size_t)a.hidden * a.rb;
        for (int r0 = 0; r0 < a.rows_per_wg; r0 += kMoeWaves) {
            const int row = row0 + r0 + wave;
            const bool live = r0 + wave < a.rows_per_wg && row < a.hidden;
            int o = 0;
            if (live) o = moe_stage_row(st, base + (size_t)row * a.rb, a.rb, lane);
            __syncthreads();
            if (live) {
                for (int c0 = beg; c0 < end;) {
                    if (end - c0 == 1) { moe_down_chunk<1>(a, st, o, n_units, lane, row, c0, end); c0 += 1; }
                    else { moe_down_chunk<kPairs>(a, st, o, n_units, lane, row, c0, end); c0 += kPairs; }
                }
            }
            __syncthreads();
        }
    }
    __threadfence();
    __syncthreads();
    // this workgroup's rows of every token: resid + the K products in ascending k, one thread per output element
    int nr = a.hidden - row0;
    if (nr > a.rows_per_wg) nr = a.rows_per_wg;
    for (int i = threadIdx.x; i < a.T * nr; i += blockDim.x) {
        const int t = i / nr, row = row0 + i % nr;
        float s = 0.0f;
        for (int k = 0; k < a.K; ++k) {
            const int p = t * a.K + k, e = a.ids[p];
            if (e >= 0 && e < a.E) s = fmaf(a.w[p], a.part[(size_t)p * a.hidden + row], s);
        }
        a.y[(size_t)t * a.hidden + row] = a.resid[(size_t)t * a.hidden + row] + s;
    }
}

static size_t moe_align256(size_t n) { return (n + 255) / 256 * 256; }
static bool moe_counts_ok(int T, int E, int K) { return T >= 1 && T <= kMoeMaxT && E >= 1 && E <= kMoeMaxE && K >= 1 && K <= kMoeMaxK && K <= E; }

}  // namespace ntk

extern "C" size_t ntk_moe_workspace_layout(int T, int E, int K, int inter, int hidden, size_t off[NTK_MOE_WS_SECTIONS]) {
    using namespace ntk;
    if (!moe_counts_ok(T, E, K) || inter <= 0 || hidden <= 0) return 0;
    const size_t pairs = (size_t)T * K;
    const size_t bytes[NTK_MOE_WS_SECTIONS] = {(size_t)T * hidden * 4, pairs * (size_t)inter * 4, pairs * (size_t)hidden * 4, pairs * 4, pairs * 4, pairs * 4,
                                               (size_t)(E + 1) * 4};
    size_t at = 0;
    for (int s = 0; s < NTK_MOE_WS_SECTIONS; ++s) {
        if (off) off[s] = at;
        at += moe_align256(bytes[s]);
    }
    return at;
}

extern "C" size_t ntk_moe_lds_bytes(int dt_a, int dt_b, int columns) {
    using namespace ntk;
    const size_t ra = moe_type_ok(dt_a) ? ntk_row_bytes(dt_a, columns) : 0, rb = dt_b < 0 ? 0 : moe_type_ok(dt_b) ? ntk_row_bytes(dt_b, columns) : 0;
    if (!ra || (dt_b >= 0 && !rb) || ra > 0x7FFFFFFFu || rb > 0x7FFFFFFFu) return 0;
    return (size_t)kMoeWaves * ((size_t)moe_image_bytes((unsigned)ra) + (dt_b < 0 ? 0 : (size_t)moe_image_bytes((unsigned)rb)));
}

extern "C" size_t ntk_moe_workspace_bytes(int T, int E, int K, int inter, int hidden) { return ntk_moe_workspace_layout(T, E, K, inter, hidden, nullptr); }

extern "C" int ntk_moe_route(const float* xn, const float* router, int T, int hidden, int E, int K, int* ids, float* w, int* offsets, int* pairs,
                             float* logits, void* stream) {
    using namespace ntk;
    if (!xn || !router || !ids || !w || !offsets || !pairs) return NTK_E_NULL;
    if (!moe_counts_ok(T, E, K) || hidden <= 0) return NTK_E_SHAPE;
    MoeRouteArgs a{xn, router, ids, w, logits, hidden, E, K, 0};
    a.vec = hidden % 4 == 0 && ((uintptr_t)xn | (uintptr_t)router) % 16 == 0 ? 1 : 0;
    hipStream_t st = resolve_stream(stream);
    hipLaunchKernelGGL(moe_route_rows_kernel, dim3((unsigned)T), dim3(256), 0, st, a);
    hipLaunchKernelGGL(moe_route_list_kernel, dim3(1), dim3(256), 0, st, (const int*)ids, offsets, pairs, T * K, E);
    return last_launch_status();
}

extern "C" int ntk_moe_gate_up(float* act, const float* xn, const void* w_gate, int dt_gate, const void* w_up, int dt_up, const int* offsets,
                               const int* pairs, int T, int hidden, int inter, int E, int K, void* stream) {
    using namespace ntk;
    if (!act || !xn || !w_gate || !w_up || !offsets || !pairs) return NTK_E_NULL;
    if (!moe_type_ok(dt_gate) || !moe_type_ok(dt_up)) return NTK_E_DTYPE;
    if (!moe_counts_ok(T, E, K) || hidden <= 0 || inter <= 0) return NTK_E_SHAPE;
    const size_t rb_g = ntk_row_bytes(dt_gate, hidden), rb_u = ntk_row_bytes(dt_up, hidden);
    if (!rb_g || !rb_u) return NTK_E_SHAPE;   // columns that are not whole blocks
    if (((uintptr_t)act | (uintptr_t)xn) % 16 != 0 || ((uintptr_t)w_gate | (uintptr_t)w_up) % 2 != 0) return NTK_E_ALIGN;
    MoeGateUpArgs a{};
    a.wg = (const uint8_t*)w_gate; a.wu = (const uint8_t*)w_up; a.xn = xn; a.offsets = offsets; a.pairs = pairs; a.act = act;
    a.dt_g = dt_gate; a.dt_u = dt_up; a.rb_g = (unsigned)rb_g; a.rb_u = (unsigned)rb_u;
    a.img_g = moe_image_bytes(a.rb_g); a.img_u = moe_image_bytes(a.rb_u);
    a.hidden = hidden; a.inter = inter; a.E = E; a.K = K; a.n_pairs = T * K;
    a.rows_per_wg = T <= 16 ? kMoeWaves : 4 * kMoeWaves;   // few rows: one row per wave, more workgroups; a prompt: x is fetched once per 16 rows
    const size_t lds = (size_t)kMoeWaves * (a.img_g + a.img_u);
    if (lds > kMoeLdsMax) return NTK_E_SHAPE;
    const unsigned blocks = (unsigned)((inter + a.rows_per_wg - 1) / a.rows_per_wg);
    if (blocks > 0x7FFFFFFFu / 2) return NTK_E_SHAPE;
    hipLaunchKernelGGL(moe_gate_up_kernel, dim3(blocks, (unsigned)E), dim3(64 * kMoeWaves), lds, resolve_stream(stream), a);
    return last_launch_status();
}

extern "C" int ntk_moe_down(float* y, const float* resid, const float* act, const void* w_down, int dt_down, const int* ids, const float* w,
                            const int* offsets, const int* pairs, float* part, int T, int hidden, int inter, int E, int K, void* stream) {
    using namespace ntk;
    if (!y || !resid || !act || !w_down || !ids || !w || !offsets || !pairs || !part) return NTK_E_NULL;
    if (!moe_type_ok(dt_down)) return NTK_E_DTYPE;
    if (!moe_counts_ok(T, E, K) || hidden <= 0 || inter <= 0) return NTK_E_SHAPE;
    const size_t rb = ntk_row_bytes(dt_down, inter);
    if (!rb) return NTK_E_SHAPE;
    if ((uintptr_t)act % 16 != 0 || (uintptr_t)w_down % 2 != 0) return NTK_E_ALIGN;
    MoeDownArgs a{};
    a.wd = (const uint8_t*)w_down; a.act = act; a.ids = ids; a.w = w; a.offsets = offsets; a.pairs = pairs; a.resid = resid; a.y = y; a.part = part;
    a.dt = dt_down; a.rb = (unsigned)rb; a.img = moe_image_bytes(a.rb);
    a.hidden = hidden; a.inter = inter; a.E = E; a.K = K; a.T = T; a.n_pairs = T * K;
    a.rows_per_wg = T <= 16 ? kMoeWaves : 2 * kMoeWaves;
    const size_t lds = (size_t)kMoeWaves * a.img;
    if (lds > kMoeLdsMax) return NTK_E_SHAPE;
    const unsigned blocks = (unsigned)((hidden + a.rows_per_wg - 1) / a.rows_per_wg);
    hipLaunchKernelGGL(moe_down_kernel, dim3(blocks), dim3(64 * kMoeWaves), lds, resolve_stream(stream), a);
    return last_launch_status();
}
