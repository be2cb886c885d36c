// kv_ops.hip -- sequence operations on the KV caches: the context shift (rows move down, K re-rotated to the new positions), both cache formats.
//
// Keys are cached AFTER RoPE, so a row that moves from position p to p + delta (delta = dst0 - src0 < 0) must be rotated by delta positions:
// pair i by the angle (float)delta * freq_i * freq_scale, evaluated like the forward kernels' pos * freq * fscale.  V rows move byte for byte.
//
// Overlap.  When n_rows > src0 - dst0 the source and destination ranges overlap, and the workgroups of a launch run in no order.  The form taken here
// needs neither a chunk loop nor a staging buffer: with step = src0 - dst0, row r of the move is READ at src0 + r and WRITTEN at src0 + (r - step),
// which is where row r - step was read -- so the rows r = c, c + step, c + 2 step, ... of one residue class c form a chain that touches no address of
// any other chain.  ONE thread owns a chain (for its 32 bytes of the row) and walks it in ascending order: every write lands on a row that this same
// thread has already read, and nothing another thread reads or writes.  No ordering between threads, waves or workgroups is needed: ONE launch for
// every step >= 1.  The parallelism is min(step, n_rows) chains x the lanes of a row x layers x 2 sides -- plentiful for the move a context shift
// makes (step about n_rows), small for a step of a few rows under a long tail (step 1: one thread per 32-byte column walks all rows).
//
// Shape.  A streaming kernel: every byte is read once and written once, 16 bytes per access.  A lane keeps ONE chunk of 8 (F16) / 16 (Q8) pairs for all
// the rows it visits, so its cos / sin stay in registers: a workgroup evaluates the head's <= 64 (cos, sin) once, into 512 bytes of LDS, and every lane
// takes its own from there.  F16: a lane holds both halves of 8 pairs (two 16-byte
// pieces), head_dim / 16 lanes per head.  Q8 (head_dim 128): a lane holds two 16-byte pieces of quants, 4 lanes per head; the head is dequantised
// (half(d) * q, exact in F32), rotated and requantised block by block with the store's arithmetic (attention_q8_decode.hip.h: q8 quantiser) -- a
// 32-block lies in two neighbouring lanes (NeoX pairing) or in one (interleaved), so the block maximum is one lane exchange at the most.
#include "common.hip.h"
#include "kv_layout.h"

namespace ntk {

typedef uint32_t kvu32x4 __attribute__((ext_vector_type(4)));

// the frequency of pair i: the table when given, else the forward kernels' expression (attention.hip)
__device__ __forceinline__ float kv_pair_freq(const float* __restrict__ inv_freq, int i, int head_dim, float theta) {
    return inv_freq ? inv_freq[i] : 1.0f / (float)pow((double)theta, (double)((2.0f * i) / head_dim));
}

struct KvShiftGeom {
    int src0, dst0, n_rows;     // rows [src0, src0 + n_rows) -> [dst0, ...)
    int step;                   // src0 - dst0 >= 1
    int chains;                 // min(step, n_rows): residue classes that hold a row
    int slots;                  // chains walked side by side (grid.x * 256 >= lanes * slots); a thread takes chains slot, slot + slots, ...
    int lanes;                  // lanes of a row: n_kv_heads * lanes per head
};

// cos | sin of the shift's angle for the head_dim / 2 (<= 64) pairs, once per workgroup (every thread of the workgroup must call); a V workgroup rotates
// nothing and gets the identity
__device__ __forceinline__ void kv_shift_table(float (&tab)[2][64], const bool is_k, const KvShiftGeom& g, const int head_dim,
                                               const float* __restrict__ inv_freq, const float theta, const float fscale) {
    const int i = threadIdx.x;
    if (i < 64) {
        float c = 1.0f, s = 0.0f;
        if (is_k && i < head_dim / 2) {
            const float angle = (float)(g.dst0 - g.src0) * kv_pair_freq(inv_freq, i, head_dim, theta) * fscale;
            c = cosf(angle);
            s = sinf(angle);
        }
        tab[0][i] = c;
        tab[1][i] = s;
    }
    __syncthreads();
}

// ---- F16: [L][max_seq][n_kv][hd] halves.  grid (x, layer, side: 0 = K, 1 = V).  LPH = hd / 16 lanes per head; lane j of a head: pairs 8 j .. 8 j + 7,
//      pieces at halves 8 j and hd / 2 + 8 j (NeoX pairing) or 16 j and 16 j + 8 (interleaved) ----
template <bool interleaved>
__global__ __launch_bounds__(256) void kv_shift_f16_kernel(uint16_t* k_cache, uint16_t* v_cache, const KvShiftGeom g, const int max_seq, const int head_dim,
                                                           const float* __restrict__ inv_freq, const float theta, const float fscale) {
    __shared__ float tab[2][64];   // cos | sin of the head's pairs: one evaluation per workgroup
    const bool is_k = blockIdx.z == 0;
    kv_shift_table(tab, is_k, g, head_dim, inv_freq, theta, fscale);
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    const int slot = (int)(gid / g.lanes), w = (int)(gid % g.lanes);
    if (slot >= g.slots) return;
    const int lph = head_dim / 16, head = w / lph, j = w % lph;
    const size_t per = (size_t)(g.lanes / lph) * head_dim;   // halves of a row
    uint16_t* const base = (is_k ? k_cache : v_cache) + (size_t)blockIdx.y * max_seq * per + (size_t)head * head_dim;
    const int o0 = interleaved ? 16 * j : 8 * j, o1 = interleaved ? 16 * j + 8 : head_dim / 2 + 8 * j;
    float cs[8], sn[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) { cs[e] = tab[0][8 * j + e]; sn[e] = tab[1][8 * j + e]; }
    for (int c = slot; c < g.chains; c += g.slots) {
        for (int r = c; r < g.n_rows; r += g.step) {   // ascending: the write of row r lands where this thread read row r - step
            const uint16_t* src = base + (size_t)(g.src0 + r) * per;
            uint16_t* dst = base + (size_t)(g.dst0 + r) * per;
            kvu32x4 p0 = *reinterpret_cast<const kvu32x4*>(src + o0);
            kvu32x4 p1 = *reinterpret_cast<const kvu32x4*>(src + o1);
            if (is_k) {
                if (interleaved) {   // piece 0: pairs 8 j + 0 .. 3 as (lo, hi) halves of a dword; piece 1: pairs 8 j + 4 .. 7
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float ra, rb;
                        rope_rotate(h2f((uint16_t)(p0[e] & 0xFFFFu)), h2f((uint16_t)(p0[e] >> 16)), cs[e], sn[e], ra, rb);
                        p0[e] = (uint32_t)f2h(ra) | ((uint32_t)f2h(rb) << 16);
                        rope_rotate(h2f((uint16_t)(p1[e] & 0xFFFFu)), h2f((uint16_t)(p1[e] >> 16)), cs[4 + e], sn[4 + e], ra, rb);
                        p1[e] = (uint32_t)f2h(ra) | ((uint32_t)f2h(rb) << 16);
                    }
                } else {             // element e of piece 0 pairs with element e of piece 1
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        float a0, b0, a1, b1;
                        rope_rotate(h2f((uint16_t)(p0[e] & 0xFFFFu)), h2f((uint16_t)(p1[e] & 0xFFFFu)), cs[2 * e], sn[2 * e], a0, b0);
                        rope_rotate(h2f((uint16_t)(p0[e] >> 16)), h2f((uint16_t)(p1[e] >> 16)), cs[2 * e + 1], sn[2 * e + 1], a1, b1);
                        p0[e] = (uint32_t)f2h(a0) | ((uint32_t)f2h(a1) << 16);
                        p1[e] = (uint32_t)f2h(b0) | ((uint32_t)f2h(b1) << 16);
                    }
                }
            }
            *reinterpret_cast<kvu32x4*>(dst + o0) = p0;
            *reinterpret_cast<kvu32x4*>(dst + o1) = p1;
        }
    }
}

// ---- Q8 (head_dim 128): per layer int8 quants [max_seq][per], then half scales [max_seq][per / 32].  4 lanes per head; lane j: pairs 16 j .. 16 j + 15,
//      pieces at elements 16 j and 64 + 16 j (NeoX pairing: blocks j / 2 and 2 + j / 2, each shared with lane j ^ 1) or 32 j and 32 j + 16 (interleaved:
//      both in block j) ----
__device__ __forceinline__ void q8_unpack16(const kvu32x4 p, const float d, float (&x)[16]) {
#pragma unroll
    for (int e = 0; e < 16; ++e) x[e] = d * sb2f(p[e >> 2], e & 3);   // half(d) * q: exact in F32
}
// one 32-block's quantisation given its amax (ggml quantize_row_q8_0_ref; the pinned undefined cases of attention_q8_decode.hip.h)
__device__ __forceinline__ kvu32x4 q8_pack16(const float (&x)[16], const float amax, uint16_t& dh) {
    const float d = amax / 127.0f;                 // IEEE division (-fhip-fp32-correctly-rounded-divide-sqrt: Makefile)
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    kvu32x4 p = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        float t = x[e] * id;
        t = t != t ? 0.0f : t;
        t = fminf(fmaxf(t, -127.0f), 127.0f);
        p[e >> 2] |= ((uint32_t)(int)roundf(t) & 0xFFu) << (8 * (e & 3));
    }
    dh = f2h(d);
    return p;
}
__device__ __forceinline__ float amax16(const float (&x)[16]) {
    float m = 0.0f;
#pragma unroll
    for (int e = 0; e < 16; ++e) m = fmaxf(m, fabsf(x[e]));
    return m;
}

template <bool interleaved>
__global__ __launch_bounds__(256) void kv_shift_q8_kernel(uint8_t* k_cache, uint8_t* v_cache, const size_t layer_bytes, const KvShiftGeom g, const int max_seq,
                                                          const float* __restrict__ inv_freq, const float theta, const float fscale) {
    constexpr int HD = 128;
    __shared__ float tab[2][64];
    const bool is_k = blockIdx.z == 0;
    kv_shift_table(tab, is_k, g, HD, inv_freq, theta, fscale);
    const size_t gid = (size_t)blockIdx.x * 256 + threadIdx.x;
    // (no early return: lane j exchanges its block maxima with lane j ^ 1, and 4 divides 256 and lanes, so the two are live or idle together)
    const int slot = (int)(gid / g.lanes), w = (int)(gid % g.lanes);
    const bool live = slot < g.slots;
    const int head = w / 4, j = w % 4;
    const size_t per = (size_t)(g.lanes / 4) * HD;   // elements of a row
    uint8_t* const layer = (is_k ? k_cache : v_cache) + (size_t)blockIdx.y * layer_bytes;
    uint8_t* const qbase = layer + (size_t)head * HD;
    uint16_t* const sbase = reinterpret_cast<uint16_t*>(layer + kv_q8_scale_offset(max_seq, per)) + (size_t)head * 4;
    const int o0 = interleaved ? 32 * j : 16 * j, o1 = interleaved ? 32 * j + 16 : 64 + 16 * j;
    const int b0 = o0 / 32, b1 = o1 / 32;
    float cs[16], sn[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) { cs[e] = tab[0][16 * j + e]; sn[e] = tab[1][16 * j + e]; }
    const int first = live ? slot : g.chains;
    for (int c = first; c < g.chains; c += g.slots) {
        for (int r = c; r < g.n_rows; r += g.step) {   // ascending (see the F16 kernel); lanes j and j ^ 1 walk the same rows
            const size_t srow = (size_t)(g.src0 + r), drow = (size_t)(g.dst0 + r);
            kvu32x4 p0 = *reinterpret_cast<const kvu32x4*>(qbase + srow * per + o0);
            kvu32x4 p1 = *reinterpret_cast<const kvu32x4*>(qbase + srow * per + o1);
            const uint16_t* ssrc = sbase + srow * (per / 32);
            uint16_t* sdst = sbase + drow * (per / 32);
            if (!is_k) {   // V: quants and scales as they are (lane j carries scale j of the head)
                const uint16_t d = ssrc[j];
                *reinterpret_cast<kvu32x4*>(qbase + drow * per + o0) = p0;
                *reinterpret_cast<kvu32x4*>(qbase + drow * per + o1) = p1;
                sdst[j] = d;
                continue;
            }
            float x0[16], x1[16];
            q8_unpack16(p0, h2f(ssrc[b0]), x0);
            q8_unpack16(p1, h2f(ssrc[b1]), x1);
            float m0, m1;
            if (interleaved) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    rope_rotate(x0[2 * e], x0[2 * e + 1], cs[e], sn[e], x0[2 * e], x0[2 * e + 1]);
                    rope_rotate(x1[2 * e], x1[2 * e + 1], cs[8 + e], sn[8 + e], x1[2 * e], x1[2 * e + 1]);
                }
                m0 = m1 = fmaxf(amax16(x0), amax16(x1));   // both pieces lie in block j
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) rope_rotate(x0[e], x1[e], cs[e], sn[e], x0[e], x1[e]);
                m0 = amax16(x0);
                m1 = amax16(x1);
                m0 = fmaxf(m0, __shfl_xor(m0, 1, 64));     // the other half of each block is lane j ^ 1's
                m1 = fmaxf(m1, __shfl_xor(m1, 1, 64));
            }
            uint16_t d0, d1;
            p0 = q8_pack16(x0, m0, d0);
            p1 = q8_pack16(x1, m1, d1);
            *reinterpret_cast<kvu32x4*>(qbase + drow * per + o0) = p0;
            *reinterpret_cast<kvu32x4*>(qbase + drow * per + o1) = p1;
            if (interleaved) sdst[b0] = d0;
            else if ((j & 1) == 0) { sdst[b0] = d0; sdst[b1] = d1; }
        }
    }
}

// the arguments both entry points share; fills g (lanes_per_head: 16-byte-pair lanes of a head)
static int kv_shift_geom(KvShiftGeom& g, dim3& grid, int n_layers, int max_seq, int n_kv_heads, int lanes_per_head, int src0, int dst0, int n_rows) {
    if (n_layers < 1 || n_layers > 65535 || max_seq < 1 || max_seq > (1 << 30) || n_kv_heads < 1) return NTK_E_SHAPE;   // (row + step stays an int)
    if (n_rows < 1 || dst0 < 0 || dst0 >= src0 || src0 >= max_seq || n_rows > max_seq - src0) return NTK_E_SHAPE;
    if ((size_t)n_kv_heads * lanes_per_head > 0x7FFFFFFFull / 256) return NTK_E_SHAPE;
    g.src0 = src0; g.dst0 = dst0; g.n_rows = n_rows;
    g.step = src0 - dst0;
    g.chains = g.step < n_rows ? g.step : n_rows;
    g.lanes = n_kv_heads * lanes_per_head;
    // chains side by side: all of them up to about two million threads in the launch, so that a thread of a long move keeps its cos / sin for many rows
    const size_t per_slot = (size_t)g.lanes * n_layers * 2;
    const size_t want = ((size_t)1 << 21) / per_slot;
    g.slots = (int)(want < 1 ? 1 : want > (size_t)g.chains ? (size_t)g.chains : want);
    const size_t threads = (size_t)g.lanes * g.slots;
    grid = dim3((unsigned)((threads + 255) / 256), (unsigned)n_layers, 2);
    return NTK_OK;
}

}  // namespace ntk

extern "C" {

int ntk_kv_shift(uint16_t* k_cache, uint16_t* v_cache, int n_layers, int max_seq, int n_kv_heads, int head_dim, int src0, int dst0, int n_rows,
                 const float* inv_freq, float theta_base, float freq_scale, int interleaved, void* stream) {
    if (!k_cache || !v_cache) return NTK_E_NULL;
    if (head_dim != 64 && head_dim != 80 && head_dim != 128) return NTK_E_SHAPE;
    ntk::KvShiftGeom g;
    dim3 grid;
    const int rc = ntk::kv_shift_geom(g, grid, n_layers, max_seq, n_kv_heads, head_dim / 16, src0, dst0, n_rows);
    if (rc != NTK_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(k_cache) & 15) || (reinterpret_cast<uintptr_t>(v_cache) & 15)) return NTK_E_ALIGN;
    hipLaunchKernelGGL(interleaved ? ntk::kv_shift_f16_kernel<true> : ntk::kv_shift_f16_kernel<false>, grid, dim3(256), 0, ntk::resolve_stream(stream),
                       k_cache, v_cache, g, max_seq, head_dim, inv_freq, theta_base, freq_scale);
    return ntk::last_launch_status();
}

int ntk_kv_shift_q8(void* k_cache_q8, void* v_cache_q8, int n_layers, int max_seq, int n_kv_heads, int head_dim, int src0, int dst0, int n_rows,
                    const float* inv_freq, float theta_base, float freq_scale, int interleaved, void* stream) {
    if (!k_cache_q8 || !v_cache_q8) return NTK_E_NULL;
    if (head_dim != 128) return NTK_E_SHAPE;   // the 8-bit store's limit
    ntk::KvShiftGeom g;
    dim3 grid;
    const int rc = ntk::kv_shift_geom(g, grid, n_layers, max_seq, n_kv_heads, 4, src0, dst0, n_rows);
    if (rc != NTK_OK) return rc;
    if ((reinterpret_cast<uintptr_t>(k_cache_q8) & 15) || (reinterpret_cast<uintptr_t>(v_cache_q8) & 15)) return NTK_E_ALIGN;
    const size_t layer_bytes = ntk::kv_q8_layer_bytes(max_seq, n_kv_heads, head_dim);
    hipLaunchKernelGGL(interleaved ? ntk::kv_shift_q8_kernel<true> : ntk::kv_shift_q8_kernel<false>, grid, dim3(256), 0, ntk::resolve_stream(stream),
                       static_cast<uint8_t*>(k_cache_q8), static_cast<uint8_t*>(v_cache_q8), layer_bytes, g, max_seq, inv_freq, theta_base, freq_scale);
    return ntk::last_launch_status();
}

}  // extern "C"
