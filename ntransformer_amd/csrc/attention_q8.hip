// attention_q8.hip -- the 8-bit (Q8_0) KV cache: store, decode attention on the matrix cores, dequantisation for the prompt path.
//
// Format.  A cache row holds Q8_0 values along head_dim: 32 consecutive elements of a head's row share one IEEE-half scale d and carry
// 32 int8 q (GGUF block_q8_0 arithmetic, ggml quantize_row_q8_0_ref in F32: amax over the block, d = amax / 127 (IEEE division),
// id = d ? 1 / d : 0, q = roundf(x * id), d stored as RNE half).  Where ggml's arithmetic is undefined (a subnormal amax makes 1 / d
// infinite) the value is pinned: x * id = NaN -> 0, then clamped to [-127, 127] before the rounding -- no defined case is changed.
// The input is the F32 post-RoPE k / the F32 v: nothing is rounded to half on the way.
//
// Device layout (the engine's own; computed in kv_layout.h and nowhere else): one layer's K (or V) cache is ONE buffer of ntk_kv_q8_cache_bytes bytes --
//   quants  int8 [max_seq][n_kv_heads * head_dim]        at byte 0          (a head's row = 128 bytes at head_dim 128: 16-byte pieces)
//   scales  half [max_seq][n_kv_heads * head_dim / 32]   at byte max_seq * n_kv_heads * head_dim
// = 1.0625 bytes per element.  The canonical 34-byte blocks exist at the API boundary only (ntransformer_amd/kv_q8.py, nt_engine_debug_kv_*_q8).
//
// Exactness.  half(d) * q is exact in F32 (11 x 8 significant bits), and the decode kernel uses exactly that value: int8 -> F16 is exact, so
//   S[key][head]  = sum over the four 32-dim blocks b of  d_b[key] * MFMA(q_b as F16, (q scale) as F16 hi + lo)     (F32 scale-FMA per block)
//   O[dim][head] += MFMA(v_q * 2^de as F16, (p * dm) as F16 hi + lo)    with d_blk(dim)[key] = dm * 2^de, both exact    (the scale folded in per dim block)
// -- the per-32-column scale-FMA structure of the prompt GEMM's Q8_0 form.  Nothing is ever rounded to half(d * q): quantisation is the only
// error the 8-bit cache adds to the F16 kernels' arithmetic, and it is pinned bit for bit by the store tests.
#include "common.hip.h"
#include "attention_merge.hip.h"
#include "attention_q8_decode.hip.h"   // the quantiser, the int8 -> F16 helpers and the decode attention's body
#include "kv_layout.h"

namespace ntk {

int launch_attention_split_combine(float* output, const float* part, int n_heads, int hd, int nsplit, int n_kv_heads, hipStream_t st);   // attention.hip
int launch_attention_batch_combine(float* output, const float* part, size_t part_row, int n_heads, int n_rows, int hd, int nsplit, int n_kv_heads,
                                   hipStream_t st);   // attention_batch.hip

// ---- ntk_kv_store_q8: one element per thread, rows [start_pos, start_pos + T) ----
__global__ __launch_bounds__(256) void kv_store_q8_kernel(int8_t* __restrict__ kq, uint16_t* __restrict__ ks, int8_t* __restrict__ vq,
                                                          uint16_t* __restrict__ vs, const float* __restrict__ k, const float* __restrict__ v,
                                                          const size_t total, const int per, const int start_pos, const int max_seq) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;   // total % 32 == 0: a block of 32 lanes is inside or outside as a whole
    const bool in = idx < total;
    const size_t src = in ? idx : 0;
    const float xk = k[src], xv = v[src];
    int8_t qk, qv;
    uint16_t dk, dv;
    q8_quantise_lane(xk, qk, dk);
    q8_quantise_lane(xv, qv, dv);
    if (!in) return;
    const size_t t = idx / per, e = idx % per;
    const size_t cp = (size_t)start_pos + t;
    if (cp >= (size_t)max_seq) return;   // reference attention.cu:336
    kq[cp * per + e] = qk;
    vq[cp * per + e] = qv;
    if ((e & 31) == 0) { ks[cp * (per / 32) + e / 32] = dk; vs[cp * (per / 32) + e / 32] = dv; }
}

// ---- ntk_rope_kv_store_q8: rope_kv_store_rows_kernel (attention.hip) with the 8-bit store; q rotated in place, the rotated k row through LDS ----
__global__ __launch_bounds__(256) void rope_kv_store_q8_rows_kernel(float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                    const int* __restrict__ positions, int n_heads, int n_kv_heads, int head_dim,
                                                                    float theta, float fscale, int interleaved, int8_t* __restrict__ kq,
                                                                    uint16_t* __restrict__ ks, int8_t* __restrict__ vq, uint16_t* __restrict__ vs,
                                                                    int start_pos, int max_seq, const float* __restrict__ inv_freq) {
    __shared__ float cs[2][128];
    extern __shared__ __attribute__((aligned(16))) float krot[];   // [n_kv_heads * head_dim]
    const int sp = blockIdx.x, half_dim = head_dim / 2;
    const int pos = positions[sp];
    for (int i = threadIdx.x; i < half_dim; i += blockDim.x) {
        const float freq = rope_freq(inv_freq, i, head_dim, theta);
        const float angle = pos * freq * fscale;
        cs[0][i] = cosf(angle);
        cs[1][i] = sinf(angle);
    }
    __syncthreads();
    const int cp = start_pos + sp, per = n_kv_heads * head_dim;
    const bool store = cp < max_seq;   // reference attention.cu:336
    const int total = (n_heads + n_kv_heads) * half_dim;
    for (int idx = threadIdx.x; idx < total; idx += blockDim.x) {
        const int pair = idx % half_dim, head = idx / half_dim;
        const int i0 = interleaved ? 2 * pair : pair, i1 = interleaved ? 2 * pair + 1 : pair + half_dim;
        const float c = cs[0][pair], sn = cs[1][pair];
        if (head < n_heads) {
            float* data = q + ((size_t)sp * n_heads + head) * head_dim;
            const float a = data[i0], b = data[i1];
            rope_rotate(a, b, c, sn, data[i0], data[i1]);
        } else {
            const int kh = head - n_heads;
            const float* data = k + ((size_t)sp * n_kv_heads + kh) * head_dim;
            rope_rotate(data[i0], data[i1], c, sn, krot[kh * head_dim + i0], krot[kh * head_dim + i1]);
        }
    }
    __syncthreads();
    for (int base = 0; base < per; base += 256) {   // (uniform trip count: every lane takes part in the block reductions)
        const int e = base + (int)threadIdx.x;
        const bool in = e < per;
        const float xk = in ? krot[e] : 0.0f, xv = in ? v[(size_t)sp * per + e] : 0.0f;
        int8_t qk, qv;
        uint16_t dk, dv;
        q8_quantise_lane(xk, qk, dk);
        q8_quantise_lane(xv, qv, dv);
        if (in && store) {
            kq[(size_t)cp * per + e] = qk;
            vq[(size_t)cp * per + e] = qv;
            if ((e & 31) == 0) { ks[(size_t)cp * (per / 32) + e / 32] = dk; vs[(size_t)cp * (per / 32) + e / 32] = dv; }
        }
    }
}

// ---- ntk_kv_dequant_q8_f16: rows [0, n) -> F16 images [n][per]: half_rne(half(d) * q); 8 elements per thread ----
__global__ __launch_bounds__(256) void kv_dequant_q8_f16_kernel(uint16_t* __restrict__ k16, uint16_t* __restrict__ v16, const int8_t* __restrict__ kq,
                                                                const uint16_t* __restrict__ ks, const int8_t* __restrict__ vq,
                                                                const uint16_t* __restrict__ vs, const size_t total8) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total8) return;
    auto one = [&](uint16_t* out, const int8_t* qp, const uint16_t* sp) {
        const u32x2 w = *reinterpret_cast<const u32x2*>(qp + 8 * idx);
        const float d = h2f(sp[idx / 4]);
        u32x4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t src = j < 2 ? w.x : w.y;
            const uint32_t a = f2h(d * sb2f(src, 2 * (j & 1))), b = f2h(d * sb2f(src, 2 * (j & 1) + 1));
            r[j] = a | (b << 16);
        }
        *reinterpret_cast<u32x4*>(out + 8 * idx) = r;
    };
    one(k16, kq, ks);
    one(v16, vq, vs);
}

// ---- ntk_attention_decode_q8: the body is attention_decode_q8_row (attention_q8_decode.hip.h); grid (n_kv_heads, nsplit) ----
__global__ __launch_bounds__(256) void attention_decode_q8_kernel(
    float* __restrict__ part, const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    int8_t* __restrict__ kq, uint16_t* __restrict__ ks, int8_t* __restrict__ vq, uint16_t* __restrict__ vs, const int* __restrict__ d_pos,
    const float* __restrict__ inv_freq, const int n_heads, const int n_kv_heads, const int max_seq, const float scale, const float theta,
    const float fscale) {
    attention_decode_q8_row(part, q, k, v, kq, ks, vq, vs, d_pos, inv_freq, n_heads, n_kv_heads, max_seq, scale, theta, fscale, (int)blockIdx.x,
                            (int)blockIdx.y, (int)gridDim.y);
}

// ---- ntk_attention_decode_q8_batch: the same body with a row dimension, grid (n_kv_heads, nsplit, B).  Row b: q / k / v at row b of the [B][..]
//      arrays, its position from positions + b, its two cache base pointers from a table passed BY VALUE in the kernel arguments (attention_batch.hip's
//      BatchCaches: no device table to write per layer), the scale planes at max_seq * per bytes behind the quants (q8_planes below), its partial
//      states at part + b * part_row.  A row's result depends on nothing but that row; the only cache bytes written are the B new rows. ----
struct Q8BatchCaches {
    uint8_t* k[NTK_ATTN_BATCH_MAX];
    uint8_t* v[NTK_ATTN_BATCH_MAX];
};
__global__ __launch_bounds__(256) void attention_batch_q8_kernel(float* __restrict__ part, const size_t part_row, const float* __restrict__ q,
                                                                 const float* __restrict__ k, const float* __restrict__ v, const Q8BatchCaches caches,
                                                                 const int* __restrict__ positions, const float* __restrict__ inv_freq,
                                                                 const int n_heads, const int n_kv_heads, const int max_seq, const float scale,
                                                                 const float theta, const float fscale) {
    const int b = blockIdx.z;
    const size_t per = (size_t)n_kv_heads * Q8_HD, planes = kv_q8_scale_offset(max_seq, per);
    uint8_t* const kc = caches.k[b];
    uint8_t* const vc = caches.v[b];
    attention_decode_q8_row(part + (size_t)b * part_row, q + (size_t)b * n_heads * Q8_HD, k + (size_t)b * per, v + (size_t)b * per,
                            reinterpret_cast<int8_t*>(kc), reinterpret_cast<uint16_t*>(kc + planes), reinterpret_cast<int8_t*>(vc),
                            reinterpret_cast<uint16_t*>(vc + planes), positions + b, inv_freq, n_heads, n_kv_heads, max_seq, scale, theta, fscale,
                            (int)blockIdx.x, (int)blockIdx.y, (int)gridDim.y);
}

struct Q8Planes {
    int8_t* q;
    uint16_t* s;
};
static Q8Planes q8_planes(void* cache, int max_seq, int per) {
    uint8_t* b = static_cast<uint8_t*>(cache);
    return {reinterpret_cast<int8_t*>(b), reinterpret_cast<uint16_t*>(b + kv_q8_scale_offset(max_seq, (size_t)per))};
}

}  // namespace ntk

extern "C" {

size_t ntk_kv_q8_cache_bytes(int max_seq, int n_kv_heads, int head_dim) {
    return ntk::kv_q8_layer_bytes(max_seq, n_kv_heads, head_dim);
}

int ntk_kv_store_q8(void* k_cache, void* v_cache, const float* k, const float* v, int seq_len, int n_kv_heads, int head_dim, int start_pos,
                    int max_seq, void* stream) {
    if (!k_cache || !v_cache || !k || !v) return NTK_E_NULL;
    if (seq_len < 0 || n_kv_heads <= 0 || head_dim <= 0 || head_dim % 32 != 0 || start_pos < 0 || max_seq <= 0) return NTK_E_SHAPE;
    const int per = n_kv_heads * head_dim;
    const size_t total = (size_t)seq_len * per;
    if (total == 0) return NTK_OK;
    if ((total + 255) / 256 > 0x7FFFFFFFull) return NTK_E_SHAPE;
    const ntk::Q8Planes kp = ntk::q8_planes(k_cache, max_seq, per), vp = ntk::q8_planes(v_cache, max_seq, per);
    hipLaunchKernelGGL(ntk::kv_store_q8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, ntk::resolve_stream(stream), kp.q, kp.s, vp.q,
                       vp.s, k, v, total, per, start_pos, max_seq);
    return ntk::last_launch_status();
}

int ntk_rope_kv_store_q8(float* q, const float* k, const float* v, const int* positions, int seq_len, int n_heads, int n_kv_heads, int head_dim,
                         float theta_base, float freq_scale, int interleaved, void* k_cache, void* v_cache, int start_pos, int max_seq,
                         void* stream) {
    return ntk_rope_kv_store_q8_tab(q, k, v, positions, seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale, interleaved, k_cache, v_cache,
                                    start_pos, max_seq, nullptr, stream);
}

// ... with the per-pair frequencies from the device table inv_freq [head_dim / 2] (NULL: the in-kernel frequency)
int ntk_rope_kv_store_q8_tab(float* q, const float* k, const float* v, const int* positions, int seq_len, int n_heads, int n_kv_heads, int head_dim,
                             float theta_base, float freq_scale, int interleaved, void* k_cache, void* v_cache, int start_pos, int max_seq,
                             const float* inv_freq, void* stream) {
    if (!q || !k || !v || !positions || !k_cache || !v_cache) return NTK_E_NULL;
    if (seq_len < 0 || n_heads <= 0 || n_kv_heads <= 0 || head_dim <= 0 || head_dim % 32 != 0 || head_dim > 256 || start_pos < 0 || max_seq <= 0)
        return NTK_E_SHAPE;
    const int per = n_kv_heads * head_dim;
    if ((size_t)per * 4 > 48 * 1024) return NTK_E_SHAPE;   // the rotated k row goes through LDS
    if (seq_len == 0) return NTK_OK;
    const ntk::Q8Planes kp = ntk::q8_planes(k_cache, max_seq, per), vp = ntk::q8_planes(v_cache, max_seq, per);
    hipLaunchKernelGGL(ntk::rope_kv_store_q8_rows_kernel, dim3(seq_len), dim3(256), (size_t)per * 4, ntk::resolve_stream(stream), q, k, v, positions,
                       n_heads, n_kv_heads, head_dim, theta_base, freq_scale, interleaved, kp.q, kp.s, vp.q, vp.s, start_pos, max_seq, inv_freq);
    return ntk::last_launch_status();
}

int ntk_kv_dequant_q8_f16(void* k_f16, void* v_f16, const void* k_cache, const void* v_cache, int n_rows, int n_kv_heads, int head_dim,
                          int max_seq, void* stream) {
    if (!k_f16 || !v_f16 || !k_cache || !v_cache) return NTK_E_NULL;
    if (n_rows < 0 || n_rows > max_seq || n_kv_heads <= 0 || head_dim <= 0 || head_dim % 32 != 0 || max_seq <= 0) return NTK_E_SHAPE;
    if ((reinterpret_cast<uintptr_t>(k_f16) & 15) || (reinterpret_cast<uintptr_t>(v_f16) & 15) || (reinterpret_cast<uintptr_t>(k_cache) & 15) ||
        (reinterpret_cast<uintptr_t>(v_cache) & 15))
        return NTK_E_ALIGN;
    const int per = n_kv_heads * head_dim;
    const size_t total8 = (size_t)n_rows * per / 8;
    if (total8 == 0) return NTK_OK;
    if ((total8 + 255) / 256 > 0x7FFFFFFFull) return NTK_E_SHAPE;
    const ntk::Q8Planes kp = ntk::q8_planes(const_cast<void*>(k_cache), max_seq, per), vp = ntk::q8_planes(const_cast<void*>(v_cache), max_seq, per);
    hipLaunchKernelGGL(ntk::kv_dequant_q8_f16_kernel, dim3((unsigned)((total8 + 255) / 256)), dim3(256), 0, ntk::resolve_stream(stream),
                       static_cast<uint16_t*>(k_f16), static_cast<uint16_t*>(v_f16), kp.q, kp.s, vp.q, vp.s, total8);
    return ntk::last_launch_status();
}

int ntk_attention_decode_q8(float* output, const float* q, const float* k, const float* v, void* k_cache, void* v_cache, const int* d_pos,
                            const float* inv_freq, int n_heads, int n_kv_heads, int head_dim, int max_seq, float scale, float theta_base,
                            float freq_scale, int nsplit, float* scratch_all, void* stream) {
    if (!output || !q || !k || !v || !k_cache || !v_cache || !d_pos || !scratch_all) return NTK_E_NULL;
    if (n_heads <= 0 || n_kv_heads <= 0 || n_heads % n_kv_heads != 0 || max_seq <= 0 || nsplit < 1 || nsplit > 1024) return NTK_E_SHAPE;
    if (head_dim != ntk::Q8_HD || n_heads / n_kv_heads > 16) return NTK_E_SHAPE;
    if ((size_t)max_seq * n_kv_heads * head_dim >= 0xF0000000ull) return NTK_E_SHAPE;   // (32-bit row offsets inside one layer's cache)
    if ((reinterpret_cast<uintptr_t>(k_cache) & 15) || (reinterpret_cast<uintptr_t>(v_cache) & 15)) return NTK_E_ALIGN;
    hipStream_t st = ntk::resolve_stream(stream);
    float* part = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(scratch_all) + ntk::att_merge_header_bytes(n_heads));
    const int per = n_kv_heads * head_dim;
    const ntk::Q8Planes kp = ntk::q8_planes(k_cache, max_seq, per), vp = ntk::q8_planes(v_cache, max_seq, per);
    hipLaunchKernelGGL(ntk::attention_decode_q8_kernel, dim3(n_kv_heads, nsplit), dim3(256), 0, st, part, q, k, v, kp.q, kp.s, vp.q, vp.s, d_pos,
                       inv_freq, n_heads, n_kv_heads, max_seq, scale, theta_base, freq_scale);
    if (ntk::last_launch_status() != NTK_OK) return NTK_E_LAUNCH;
    return ntk::launch_attention_split_combine(output, part, n_heads, head_dim, nsplit, n_kv_heads, st);
}

int ntk_attention_decode_q8_batch(float* output, const float* q, const float* k, const float* v, const ntk_kv_batch* caches, const int* positions,
                                  int n_rows, const float* inv_freq, int n_heads, int n_kv_heads, int head_dim, int max_seq, float scale,
                                  float theta_base, float freq_scale, int nsplit, float* scratch, void* stream) {
    if (!output || !q || !k || !v || !caches || !positions || !scratch) return NTK_E_NULL;
    if (n_rows < 1 || n_rows > NTK_ATTN_BATCH_MAX) return NTK_E_SHAPE;
    if (n_heads <= 0 || n_kv_heads <= 0 || n_heads % n_kv_heads != 0 || max_seq <= 0 || nsplit < 1 || nsplit > 1024) return NTK_E_SHAPE;
    if (head_dim != ntk::Q8_HD || n_heads / n_kv_heads > 16) return NTK_E_SHAPE;
    if ((size_t)max_seq * n_kv_heads * head_dim >= 0xF0000000ull) return NTK_E_SHAPE;   // (32-bit row offsets inside one layer's cache)
    ntk::Q8BatchCaches c{};
    for (int b = 0; b < n_rows; ++b) {
        if (!caches->k[b] || !caches->v[b]) return NTK_E_NULL;
        c.k[b] = static_cast<uint8_t*>(caches->k[b]);
        c.v[b] = static_cast<uint8_t*>(caches->v[b]);
        if ((reinterpret_cast<uintptr_t>(c.k[b]) & 15) || (reinterpret_cast<uintptr_t>(c.v[b]) & 15)) return NTK_E_ALIGN;
    }
    for (int b = n_rows; b < NTK_ATTN_BATCH_MAX; ++b) { c.k[b] = c.k[0]; c.v[b] = c.v[0]; }   // (never indexed: the grid has n_rows rows)
    hipStream_t st = ntk::resolve_stream(stream);
    const size_t part_row = ntk_attention_split_scratch_bytes(n_heads, head_dim, nsplit) / sizeof(float);   // a row: counters, then states
    float* part = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(scratch) + ntk::att_merge_header_bytes(n_heads));
    hipLaunchKernelGGL(ntk::attention_batch_q8_kernel, dim3(n_kv_heads, nsplit, n_rows), dim3(256), 0, st, part, part_row, q, k, v, c, positions,
                       inv_freq, n_heads, n_kv_heads, max_seq, scale, theta_base, freq_scale);
    if (ntk::last_launch_status() != NTK_OK) return NTK_E_LAUNCH;
    return ntk::launch_attention_batch_combine(output, part, part_row, n_heads, n_rows, head_dim, nsplit, n_kv_heads, st);
}

}  // extern "C"
