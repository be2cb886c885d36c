// attention_batch.hip -- decode attention for a BATCH of sequences: B <= 16 rows, each with its own KV cache and its own position, one launch
// (+ the combine launch when it splits).  Row b is exactly what ntk_attention_decode_fused (nsplit == 1) / ntk_attention_decode_split (nsplit > 1)
// compute for one row: RoPE of q and k at positions[b], the rotated k and v stored as F16 (RNE) into row positions[b] of cache b, GQA attention over
// rows 0 .. positions[b] of cache b -- the same device functions (attention_decode.hip.h, attention_mfma_decode.hip.h, attention_merge.hip.h), so
// the same bits as the single-row launch of the same form, and a row's result depends on nothing but that row.
//
// The only thing added is a row dimension of the grid: workgroup (.., b) takes q / k / v / output at row b of the [B][..] arrays, its position from
// positions + b (the walk reads it through the same `const int* d_pos` as the single-row kernels), its cache base pointers from a table passed BY
// VALUE in the kernel arguments (2 x 16 pointers: no device table to write per layer) and its partial states from scratch + b x the single-row
// scratch.  A split that lies wholly past a row's position leaves an empty state (weight 0 in the merge), as in the single-row kernels with more
// splits than positions.  Cache rows past a row's position may be loaded (clamped to max_seq - 1) and never enter the result; the only cache rows
// written are the B rows named.  Two rows of one batch must not name the same cache (the caller checks: Model::decode_batch).
#include "common.hip.h"
#include "attention_decode.hip.h"
#include "attention_mfma_decode.hip.h"
#include "../../include/ntk_engine.h"

namespace ntk {

// the rows' cache base pointers of one layer, in the kernel arguments
struct BatchCaches {
    uint16_t* k[NTK_ATTN_BATCH_MAX];
    uint16_t* v[NTK_ATTN_BATCH_MAX];
};

// the operands of row b
struct BatchRow {
    const float *q, *k, *v;
    float* out;
    uint16_t *kc, *vc;
    const int* pos;
};
__device__ __forceinline__ BatchRow batch_row(const int b, float* output, const float* q, const float* k, const float* v, const BatchCaches& c,
                                              const int* positions, const int n_heads, const int n_kv_heads, const int hd) {
    return {q + (size_t)b * n_heads * hd, k + (size_t)b * n_kv_heads * hd, v + (size_t)b * n_kv_heads * hd, output + (size_t)b * n_heads * hd,
            c.k[b], c.v[b], positions + b};
}

// nsplit == 1, head_dim 64 / 128 / 256: the single-pass walk, grid (n_heads, B)
template <int LPR>
__global__ __launch_bounds__(256) void attention_batch_walk_kernel(float* __restrict__ output, const float* __restrict__ q, const float* __restrict__ k,
                                                                   const float* __restrict__ v, const BatchCaches caches,
                                                                   const int* __restrict__ positions, const float* __restrict__ inv_freq, int n_heads,
                                                                   int n_kv_heads, int hd, int max_seq, float scale, float theta, float fscale) {
    const BatchRow r = batch_row((int)blockIdx.y, output, q, k, v, caches, positions, n_heads, n_kv_heads, hd);
    attention_decode_walk<LPR, 4, false>(r.out, r.q, r.k, r.v, r.kc, r.vc, r.pos, inv_freq, n_heads, n_kv_heads, hd, max_seq, scale, theta, fscale,
                                         (int)blockIdx.x, 0, 1);
}

// nsplit == 1, any other head_dim: the three-pass generic form, grid (n_heads, B)
__global__ __launch_bounds__(256) void attention_batch_generic_kernel(float* __restrict__ output, const float* __restrict__ q,
                                                                      const float* __restrict__ k, const float* __restrict__ v,
                                                                      const BatchCaches caches, const int* __restrict__ positions, int n_heads,
                                                                      int n_kv_heads, int hd, int max_seq, float scale, float theta, float fscale) {
    const BatchRow r = batch_row((int)blockIdx.y, output, q, k, v, caches, positions, n_heads, n_kv_heads, hd);
    attention_decode_fused_row<0>(r.out, r.q, r.k, r.v, r.kc, r.vc, r.pos, n_heads, n_kv_heads, hd, max_seq, scale, theta, fscale, (int)blockIdx.x);
}

// nsplit > 1, the per-query-head walk: grid (n_heads, nsplit, B), the head order of attention_decode_split_kernel; part_row = floats of one row's scratch
template <int LPR>
__global__ __launch_bounds__(256) void attention_batch_split_kernel(float* __restrict__ part, size_t part_row, const float* __restrict__ q,
                                                                    const float* __restrict__ k, const float* __restrict__ v, const BatchCaches caches,
                                                                    const int* __restrict__ positions, const float* __restrict__ inv_freq,
                                                                    int n_heads, int n_kv_heads, int hd, int max_seq, float scale, float theta,
                                                                    float fscale) {
    const BatchRow r = batch_row((int)blockIdx.z, nullptr, q, k, v, caches, positions, n_heads, n_kv_heads, hd);
    const int group = n_heads / n_kv_heads;
    const int kv_head = blockIdx.x % n_kv_heads, head = kv_head * group + blockIdx.x / n_kv_heads;
    const int sp = blockIdx.y, nsplit = gridDim.y;
    attention_decode_walk<LPR, 4, true, false>(part + (size_t)blockIdx.z * part_row + ((size_t)head * nsplit + sp) * (hd + 2), r.q, r.k, r.v, r.kc, r.vc,
                                               r.pos, inv_freq, n_heads, n_kv_heads, hd, max_seq, scale, theta, fscale, head, sp, nsplit);
}

// nsplit >= 16, head_dim 128: the matrix-core form, grid (n_kv_heads, nsplit, B)
__global__ __launch_bounds__(256) void attention_batch_mfma_kernel(float* __restrict__ part, size_t part_row, const float* __restrict__ q,
                                                                   const float* __restrict__ k, const float* __restrict__ v, const BatchCaches caches,
                                                                   const int* __restrict__ positions, const float* __restrict__ inv_freq, int n_heads,
                                                                   int n_kv_heads, int max_seq, float scale, float theta, float fscale) {
    const BatchRow r = batch_row((int)blockIdx.z, nullptr, q, k, v, caches, positions, n_heads, n_kv_heads, AM_HD);
    attention_decode_kvhead_mfma<false>(part + (size_t)blockIdx.z * part_row, r.q, r.k, r.v, r.kc, r.vc, r.pos, inv_freq, n_heads, n_kv_heads, max_seq,
                                        scale, theta, fscale, nullptr, nullptr);   // (KV head, split: the grid's x and y, as in the single-row launch)
}

// the merge of the splits: grid (n_heads, B)
__global__ __launch_bounds__(128) void attention_batch_combine_kernel(float* __restrict__ output, const float* __restrict__ part, size_t part_row,
                                                                      int hd, int nsplit, int n_kv_heads) {
    attention_split_combine_head(output + (size_t)blockIdx.y * gridDim.x * hd, part + (size_t)blockIdx.y * part_row, hd, nsplit, n_kv_heads,
                                 (int)blockIdx.x, (int)gridDim.x);
}

// ... and its launcher, for the batched launch over the 8-bit caches too (attention_q8.hip), as attention.hip exposes launch_attention_split_combine
int launch_attention_batch_combine(float* output, const float* part, size_t part_row, int n_heads, int n_rows, int hd, int nsplit, int n_kv_heads,
                                   hipStream_t st) {
    hipLaunchKernelGGL(attention_batch_combine_kernel, dim3(n_heads, n_rows), dim3(128), 0, st, output, part, part_row, hd, nsplit, n_kv_heads);
    return last_launch_status();
}

}  // namespace ntk

extern "C" int ntk_attention_decode_batch(float* output, const float* q, const float* k, const float* v, const ntk_kv_batch* caches,
                                          const int* positions, int n_rows, const float* inv_freq, int n_heads, int n_kv_heads, int head_dim,
                                          int max_seq, float scale, float theta_base, float freq_scale, int nsplit, float* scratch, void* stream) {
    if (!output || !q || !k || !v || !caches || !positions) return NTK_E_NULL;
    if (n_rows < 1 || n_rows > NTK_ATTN_BATCH_MAX) return NTK_E_SHAPE;
    if (n_heads <= 0 || n_kv_heads <= 0 || n_heads % n_kv_heads != 0 || head_dim <= 0 || (head_dim & 1) || max_seq <= 0 || nsplit < 1 || nsplit > 1024)
        return NTK_E_SHAPE;
    if ((size_t)max_seq * n_kv_heads * head_dim * 2 >= 0xF0000000ull) return NTK_E_SHAPE;   // (32-bit row offsets inside one layer's cache)
    ntk::BatchCaches c{};
    bool aligned = true;
    for (int b = 0; b < n_rows; ++b) {
        if (!caches->k[b] || !caches->v[b]) return NTK_E_NULL;
        c.k[b] = static_cast<uint16_t*>(caches->k[b]);
        c.v[b] = static_cast<uint16_t*>(caches->v[b]);
        aligned = aligned && (reinterpret_cast<uintptr_t>(c.k[b]) & 15) == 0 && (reinterpret_cast<uintptr_t>(c.v[b]) & 15) == 0;
    }
    for (int b = n_rows; b < NTK_ATTN_BATCH_MAX; ++b) { c.k[b] = c.k[0]; c.v[b] = c.v[0]; }   // (never indexed: the grid has n_rows rows)
    const bool walk_hd = head_dim == 128 || head_dim == 64 || head_dim == 256;
    hipStream_t st = ntk::resolve_stream(stream);
    const int G = walk_hd ? 4 * (64 / (head_dim / 8)) : 0;
    const size_t walk_lds = sizeof(float) * ((size_t)3 * head_dim + 2 * G + (size_t)G * head_dim);
    if (nsplit == 1) {   // the forms of ntk_attention_decode_fused
        const dim3 grid(n_heads, n_rows);
        if (aligned && walk_hd) {
#define NTK_ATTB(LPR_) hipLaunchKernelGGL((ntk::attention_batch_walk_kernel<LPR_>), grid, dim3(256), walk_lds, st, output, q, k, v, c, positions, inv_freq, \
                                          n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base, freq_scale)
            if (head_dim == 128) NTK_ATTB(16);
            else if (head_dim == 64) NTK_ATTB(8);
            else NTK_ATTB(32);
#undef NTK_ATTB
            return ntk::last_launch_status();
        }
        const size_t lds = sizeof(float) * ((size_t)3 * head_dim + 16 + 4 * (size_t)head_dim + (size_t)max_seq + 1);   // (attention.hip: attn_lds)
        if (lds > 160 * 1024) return NTK_E_SHAPE;
        if (lds > 64 * 1024)
            (void)hipFuncSetAttribute(reinterpret_cast<const void*>(ntk::attention_batch_generic_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(ntk::attention_batch_generic_kernel, grid, dim3(256), lds, st, output, q, k, v, c, positions, n_heads, n_kv_heads, head_dim,
                           max_seq, scale, theta_base, freq_scale);
        return ntk::last_launch_status();
    }
    // the forms of ntk_attention_decode_split, with its refusals
    if (!scratch) return NTK_E_NULL;
    if (!walk_hd) return NTK_E_SHAPE;
    if (!aligned) return NTK_E_ALIGN;
    const size_t row_bytes = ntk_attention_split_scratch_bytes(n_heads, head_dim, nsplit), part_row = row_bytes / sizeof(float);
    float* part = reinterpret_cast<float*>(reinterpret_cast<uint8_t*>(scratch) + ntk::att_merge_header_bytes(n_heads));   // (a row: counters, then states)
    if (head_dim == 128 && n_heads / n_kv_heads <= 16 && nsplit >= 16) {
        hipLaunchKernelGGL(ntk::attention_batch_mfma_kernel, dim3(n_kv_heads, nsplit, n_rows), dim3(256), 0, st, part, part_row, q, k, v, c, positions,
                           inv_freq, n_heads, n_kv_heads, max_seq, scale, theta_base, freq_scale);
    } else {
#define NTK_ATTB(LPR_) hipLaunchKernelGGL((ntk::attention_batch_split_kernel<LPR_>), dim3(n_heads, nsplit, n_rows), dim3(256), walk_lds, st, part, part_row, \
                                          q, k, v, c, positions, inv_freq, n_heads, n_kv_heads, head_dim, max_seq, scale, theta_base, freq_scale)
        if (head_dim == 128) NTK_ATTB(16);
        else if (head_dim == 64) NTK_ATTB(8);
        else NTK_ATTB(32);
#undef NTK_ATTB
    }
    if (ntk::last_launch_status() != NTK_OK) return NTK_E_LAUNCH;
    return ntk::launch_attention_batch_combine(output, part, part_row, n_heads, n_rows, head_dim, nsplit, n_kv_heads, st);
}
