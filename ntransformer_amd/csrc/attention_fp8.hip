// attention_fp8.hip -- the FP8 KV cache: store, decode attention, the F16 image for the prompt path.
//
// Format.  A cache element is ONE byte, an OCP E4M3 code ("fn": 4 exponent bits, bias 7, 3 mantissa bits, subnormals from 2^-9, maximum 448, no
// infinities, S.1111.111 = NaN) -- what gfx950's v_cvt_pk_fp8_f32 writes.  The input is the F32 post-RoPE k / the F32 v, rounded to nearest even
// and saturated at +-448 (infinities included); NaN in, NaN out.  No scales: exactly 1 byte per element.
//
// Device layout (kv_layout.h): one layer's K (or V) cache is ONE buffer of ntk_kv_fp8_cache_bytes bytes, uint8 [max_seq][n_kv_heads * head_dim].
//
// Exactness.  E4M3 -> F16 is exact (every code is a normal half), and the decode kernel computes with exactly those halves: it IS the F16 matrix-core
// kernel (attention_mfma_decode.hip.h) over the exactly decoded cache, with q * scale and P each as an F16 value + the F16 rounding of the rest.  The
// format adds its rounding at the store and nothing afterwards; the store is pinned bit for bit by the tests.
//
// Why the rows are converted and not fed to the FP8 matrix instructions as loaded.  v_mfma_f32_16x16x32_fp8_fp8 takes BOTH operands in 8 bits, so
// the F32 query (and P) would go in as a sum of E4M3 pieces, each the RNE of the running residual under a power of two of its own.  A piece carries
// 4 significant bits, so n pieces leave a residual of 2^-4n of an ELEMENT (E4M3 is a floating format: the bound is per element, not per head).  The
// kernel's bar is 3e-5 of a unit-scale output, i.e. score errors of about 1e-5, and at the engine's scale 1 / sqrt(128) a query channel of 300 x the
// others puts a term of about 26 into a score: 1e-5 / 26 = 2^-21 of that element, so n = 6 (2^-24; n = 5 leaves 2^-20, at the bar) where the F16
// split's two pieces give 2^-22.  (At a sixteenth of that scale -- what the kernel's own test uses so that the softmax keeps a spread -- the term is
// 1.7 and n = 5: 160 passes, a tie with converting, before P's pieces, which the V side would need as well, are counted.)  Six
// pieces are 48 FP8 MFMAs of 4 passes per chunk of 32 keys for S alone (192 passes) against 16 F16 MFMAs of 8 passes (128) plus the chunk's 32
// one-pass K conversions (160 in all) -- and three accumulators per key block for the pieces' powers of two.  Three pieces (96 passes) would be
// cheaper and miss the bar by 2^12.  The scaled form v_mfma_scale_f32_16x16x128_f8f6f4 changes none of this: its block scales replace the powers of
// two, not the pieces.  So K and V take the other route: v_cvt_scalef32_pk_f16_fp8 turns two bytes into two halves in one instruction, 64 of them
// per lane and chunk, against the Q8_0 kernel's byte permutes, bias subtractions, per-32 scale FMAs and 4 x 4 byte transposes through LDS.
#include "common.hip.h"
#include "attention_merge.hip.h"
#include "attention_fp8_decode.hip.h"   // the encoder, the E4M3 -> F16 conversion and the decode attention's body
#include "kv_layout.h"

namespace ntk {

int launch_attention_split_combine(float* output, const float* part, int n_heads, int hd, int nsplit, int n_kv_heads, hipStream_t st);   // attention.hip

// ---- ntk_kv_store_fp8: four elements per thread, rows [start_pos, start_pos + T) (per % 4 == 0: a thread's four lie in one row) ----
__global__ __launch_bounds__(256) void kv_store_fp8_kernel(uint8_t* __restrict__ kc, uint8_t* __restrict__ vc, const float* __restrict__ k,
                                                           const float* __restrict__ v, const size_t total4, const int per, const int start_pos,
                                                           const int max_seq) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total4) return;
    const size_t t = (4 * idx) / per, e = (4 * idx) % per;
    const size_t cp = (size_t)start_pos + t;
    if (cp >= (size_t)max_seq) return;   // reference attention.cu:336
    const float4 a = *reinterpret_cast<const float4*>(k + 4 * idx), b = *reinterpret_cast<const float4*>(v + 4 * idx);
    *reinterpret_cast<uint32_t*>(kc + cp * per + e) = fp8_encode4(a.x, a.y, a.z, a.w);
    *reinterpret_cast<uint32_t*>(vc + cp * per + e) = fp8_encode4(b.x, b.y, b.z, b.w);
}

// ---- ntk_rope_kv_store_fp8: rope_kv_store_rows_kernel (attention.hip) with the FP8 store; q rotated in place, the rotated k row through LDS ----
__global__ __launch_bounds__(256) void rope_kv_store_fp8_rows_kernel(float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
                                                                     const int* __restrict__ positions, int n_heads, int n_kv_heads, int head_dim,
                                                                     float theta, float fscale, int interleaved, uint8_t* __restrict__ kc,
                                                                     uint8_t* __restrict__ vc, int start_pos, int max_seq,
                                                                     const float* __restrict__ inv_freq) {
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
    if (cp >= max_seq) return;   // reference attention.cu:336
    for (int e = 4 * (int)threadIdx.x; e < per; e += 4 * 256) {
        const float4 a = *reinterpret_cast<const float4*>(krot + e), b = *reinterpret_cast<const float4*>(v + (size_t)sp * per + e);
        *reinterpret_cast<uint32_t*>(kc + (size_t)cp * per + e) = fp8_encode4(a.x, a.y, a.z, a.w);
        *reinterpret_cast<uint32_t*>(vc + (size_t)cp * per + e) = fp8_encode4(b.x, b.y, b.z, b.w);
    }
}

// ---- ntk_kv_dequant_fp8_f16: rows [0, n) -> F16 images [n][per], exactly; 8 elements per thread ----
__global__ __launch_bounds__(256) void kv_dequant_fp8_f16_kernel(uint16_t* __restrict__ k16, uint16_t* __restrict__ v16, const uint8_t* __restrict__ kc,
                                                                 const uint8_t* __restrict__ vc, const size_t total8) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total8) return;
    *reinterpret_cast<u32x4*>(k16 + 8 * idx) = fp8_cvt8(*reinterpret_cast<const u32x2*>(kc + 8 * idx));
    *reinterpret_cast<u32x4*>(v16 + 8 * idx) = fp8_cvt8(*reinterpret_cast<const u32x2*>(vc + 8 * idx));
}

// ---- ntk_attention_decode_fp8: the body is attention_decode_fp8_row (attention_fp8_decode.hip.h); grid (n_kv_heads, nsplit) ----
__global__ __launch_bounds__(256) void attention_decode_fp8_kernel(float* __restrict__ part, const float* __restrict__ q, const float* __restrict__ k,
                                                                   const float* __restrict__ v, uint8_t* __restrict__ kc, uint8_t* __restrict__ vc,
                                                                   const int* __restrict__ d_pos, const float* __restrict__ inv_freq,
                                                                   const int n_heads, const int n_kv_heads, const int max_seq, const float scale,
                                                                   const float theta, const float fscale) {
    attention_decode_fp8_row(part, q, k, v, kc, vc, d_pos, inv_freq, n_heads, n_kv_heads, max_seq, scale, theta, fscale, (int)blockIdx.x,
                             (int)blockIdx.y, (int)gridDim.y);
}

static bool misaligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

}  // namespace ntk

extern "C" {

size_t ntk_kv_fp8_cache_bytes(int max_seq, int n_kv_heads, int head_dim) {
    return ntk::kv_fp8_layer_bytes(max_seq, n_kv_heads, head_dim);
}

int ntk_kv_store_fp8(void* k_cache, void* v_cache, const float* k, const float* v, int seq_len, int n_kv_heads, int head_dim, int start_pos,
                     int max_seq, void* stream) {
    if (!k_cache || !v_cache || !k || !v) return NTK_E_NULL;
    if (seq_len < 0 || n_kv_heads <= 0 || head_dim <= 0 || head_dim % 8 != 0 || start_pos < 0 || max_seq <= 0) return NTK_E_SHAPE;
    if (ntk::misaligned16(k_cache) || ntk::misaligned16(v_cache) || ntk::misaligned16(k) || ntk::misaligned16(v)) return NTK_E_ALIGN;
    const int per = n_kv_heads * head_dim;
    const size_t total4 = (size_t)seq_len * per / 4;
    if (total4 == 0) return NTK_OK;
    if ((total4 + 255) / 256 > 0x7FFFFFFFull) return NTK_E_SHAPE;
    hipLaunchKernelGGL(ntk::kv_store_fp8_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, ntk::resolve_stream(stream),
                       static_cast<uint8_t*>(k_cache), static_cast<uint8_t*>(v_cache), k, v, total4, per, start_pos, max_seq);
    return ntk::last_launch_status();
}

int ntk_rope_kv_store_fp8(float* q, const float* k, const float* v, const int* positions, int seq_len, int n_heads, int n_kv_heads, int head_dim,
                          float theta_base, float freq_scale, int interleaved, void* k_cache, void* v_cache, int start_pos, int max_seq,
                          void* stream) {
    return ntk_rope_kv_store_fp8_tab(q, k, v, positions, seq_len, n_heads, n_kv_heads, head_dim, theta_base, freq_scale, interleaved, k_cache,
                                     v_cache, start_pos, max_seq, nullptr, stream);
}

// ... with the per-pair frequencies from the device table inv_freq [head_dim / 2] (NULL: the in-kernel frequency)
int ntk_rope_kv_store_fp8_tab(float* q, const float* k, const float* v, const int* positions, int seq_len, int n_heads, int n_kv_heads, int head_dim,
                              float theta_base, float freq_scale, int interleaved, void* k_cache, void* v_cache, int start_pos, int max_seq,
                              const float* inv_freq, void* stream) {
    if (!q || !k || !v || !positions || !k_cache || !v_cache) return NTK_E_NULL;
    if (seq_len < 0 || n_heads <= 0 || n_kv_heads <= 0 || head_dim <= 0 || head_dim % 8 != 0 || head_dim > 256 || start_pos < 0 || max_seq <= 0)
        return NTK_E_SHAPE;
    if (ntk::misaligned16(k_cache) || ntk::misaligned16(v_cache) || ntk::misaligned16(v)) return NTK_E_ALIGN;
    const int per = n_kv_heads * head_dim;
    if ((size_t)per * 4 > 48 * 1024) return NTK_E_SHAPE;   // the rotated k row goes through LDS
    if (seq_len == 0) return NTK_OK;
    hipLaunchKernelGGL(ntk::rope_kv_store_fp8_rows_kernel, dim3(seq_len), dim3(256), (size_t)per * 4, ntk::resolve_stream(stream), q, k, v, positions,
                       n_heads, n_kv_heads, head_dim, theta_base, freq_scale, interleaved, static_cast<uint8_t*>(k_cache),
                       static_cast<uint8_t*>(v_cache), start_pos, max_seq, inv_freq);
    return ntk::last_launch_status();
}

int ntk_kv_dequant_fp8_f16(void* k_f16, void* v_f16, const void* k_cache, const void* v_cache, int n_rows, int n_kv_heads, int head_dim,
                           int max_seq, void* stream) {
    if (!k_f16 || !v_f16 || !k_cache || !v_cache) return NTK_E_NULL;
    if (n_rows < 0 || n_rows > max_seq || n_kv_heads <= 0 || head_dim <= 0 || head_dim % 8 != 0 || max_seq <= 0) return NTK_E_SHAPE;
    if (ntk::misaligned16(k_f16) || ntk::misaligned16(v_f16) || ntk::misaligned16(k_cache) || ntk::misaligned16(v_cache)) return NTK_E_ALIGN;
    const size_t total8 = (size_t)n_rows * n_kv_heads * head_dim / 8;
    if (total8 == 0) return NTK_OK;
    if ((total8 + 255) / 256 > 0x7FFFFFFFull) return NTK_E_SHAPE;
    hipLaunchKernelGGL(ntk::kv_dequant_fp8_f16_kernel, dim3((unsigned)((total8 + 255) / 256)), dim3(256), 0, ntk::resolve_stream(stream),
                       static_cast<uint16_t*>(k_f16), static_cast<uint16_t*>(v_f16), static_cast<const uint8_t*>(k_cache),
                       static_cast<const uint8_t*>(v_cache), total8);
    return ntk::last_launch_status();
}

int ntk_attention_decode_fp8(float* output, const float* q, const float* k, const float* v, void* k_cache, void* v_cache, const int* d_pos,
                             const float* inv_freq, int n_heads, int n_kv_heads, int head_dim, int max_seq, float scale, float theta_base,
                             float freq_scale, int nsplit, float* scratch_all, void* stream) {
    if (!output || !q || !k || !v || !k_cache || !v_cache || !d_pos || !scratch_all) return NTK_E_NULL;
    if (n_heads <= 0 || n_kv_heads <= 0 || n_heads % n_kv_heads != 0 || max_seq <= 0 || nsplit < 1 || nsplit > 1024) return NTK_E_SHAPE;
    if (head_dim != ntk::F8_HD || n_heads / n_kv_heads > 16) return NTK_E_SHAPE;
    if ((size_t)max_seq * n_kv_heads * head_dim >= 0xF0000000ull) return NTK_E_SHAPE;   // (32-bit row offsets inside one layer's cache)
    if (ntk::misaligned16(k_cache) || ntk::misaligned16(v_cache)) return NTK_E_ALIGN;
    hipStream_t st = ntk::resolve_stream(stream);
    float* part = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(scratch_all) + ntk::att_merge_header_bytes(n_heads));
    hipLaunchKernelGGL(ntk::attention_decode_fp8_kernel, dim3(n_kv_heads, nsplit), dim3(256), 0, st, part, q, k, v, static_cast<uint8_t*>(k_cache),
                       static_cast<uint8_t*>(v_cache), d_pos, inv_freq, n_heads, n_kv_heads, max_seq, scale, theta_base, freq_scale);
    if (ntk::last_launch_status() != NTK_OK) return NTK_E_LAUNCH;
    return ntk::launch_attention_split_combine(output, part, n_heads, head_dim, nsplit, n_kv_heads, st);
}

}  // extern "C"
