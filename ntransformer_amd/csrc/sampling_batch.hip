// sampling_batch.hip -- the sampler over the rows of a batched decode step (ntk_sample_rows_top_k), each row with its own settings.
//
// A batched step leaves [B][vocab] logits on the device.  Sampling them on the host costs a B x vocab download (8 MB at 16 rows of 128 256) and B
// partial sorts over the whole vocabulary per step -- the work ntk_sample_top_k took off the single-sequence path (sampling.hip).  Here every row is
// sampled by that kernel's own device code (sampling_core.hip.h), in a number of launches that does not depend on the row count:
//   1. the repeat penalty, one THREAD per row (a row's window is walked in order by one thread, as the reference does; skipped when no row has one);
//   2. stage 1 over a (chunk, row) grid: the chunk's 64 best of logit / temperature -- or, for a greedy row, the chunk's first maximum alone;
//   3. stage 2, one workgroup per row: the survivors sorted, softmax / top-p / the cumulative walk against the row's draw by one thread -- or the
//      first maximum over the chunks' maxima.
// A workgroup reads and writes its own row only, so a row's result does not depend on its companions or on where in the batch it stands.
#include "sampling_core.hip.h"

namespace ntk {

__global__ void sample_rows_penalty_kernel(float* __restrict__ logits, int n_rows, int vocab, int ld, const int* __restrict__ recent, int recent_ld,
                                           const ntk_sample_rows rows) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_rows || !(rows.repeat_penalty[b] > 1.0f) || rows.n_recent[b] <= 0) return;
    sk_penalty(logits + (size_t)b * ld, vocab, recent + (size_t)b * recent_ld, rows.n_recent[b], rows.repeat_penalty[b]);
}

__global__ __launch_bounds__(1024) void sample_rows_stage1(const float* __restrict__ logits, int vocab, int ld, const ntk_sample_rows rows,
                                                           unsigned long long* __restrict__ cand, int cand_ld) {
    __shared__ unsigned long long keys[SK_CHUNK];
    const int b = blockIdx.y;
    const float* row = logits + (size_t)b * ld;
    unsigned long long* out = cand + (size_t)b * cand_ld;
    const float t = rows.temperature[b];
    if (t > 0.0f) sk_stage1(row, vocab, t, blockIdx.x, out, keys);
    else sk_stage1_greedy(row, vocab, blockIdx.x, out, keys);
}

__global__ __launch_bounds__(1024) void sample_rows_stage2(const unsigned long long* __restrict__ cand, int cand_ld, int chunks, int vocab,
                                                           const ntk_sample_rows rows, int* __restrict__ d_out, int* __restrict__ h_mirror) {
    __shared__ unsigned long long keys[SK_MAXCAND];
    const int b = blockIdx.x;
    const unsigned long long* in = cand + (size_t)b * cand_ld;
    int* mirror = h_mirror ? h_mirror + b : nullptr;
    if (rows.temperature[b] > 0.0f) {
        const int top_k = rows.top_k[b] < vocab ? rows.top_k[b] : vocab;
        sk_stage2(in, chunks * SK_KEEP, top_k, rows.top_p[b], rows.r[b], d_out + b, mirror, keys);
    } else {
        sk_stage2_greedy(in, chunks, d_out + b, mirror, keys);
    }
}

}  // namespace ntk

extern "C" {

using namespace ntk;

size_t ntk_sample_rows_scratch_bytes(int n_rows, int vocab) {
    if (n_rows < 1 || vocab < 1) return 256;
    const size_t chunks = ((size_t)vocab + SK_CHUNK - 1) / SK_CHUNK;
    return (size_t)n_rows * chunks * SK_KEEP * sizeof(unsigned long long) + 256;
}

int ntk_sample_rows_top_k(float* logits, int n_rows, int vocab, int ld, const int* d_recent, int recent_ld, const ntk_sample_rows* rows, int* d_out,
                          int* h_mirror, void* scratch, void* stream) {
    if (!logits || !rows || !d_out || !scratch) return NTK_E_NULL;
    if (n_rows < 1 || n_rows > NTK_SAMPLE_ROWS_MAX || vocab < 1 || ld < vocab || recent_ld < 0) return NTK_E_SHAPE;
    const int chunks = (vocab + SK_CHUNK - 1) / SK_CHUNK;
    if (chunks * SK_KEEP > SK_MAXCAND) return NTK_E_SHAPE;   // vocabularies beyond 131 072
    bool penalty = false;
    for (int b = 0; b < n_rows; ++b) {
        if (rows->temperature[b] > 0.0f && (rows->top_k[b] < 1 || rows->top_k[b] > SK_KEEP)) return NTK_E_SHAPE;   // wider top-k: the host sampler
        if (rows->n_recent[b] < 0 || rows->n_recent[b] > recent_ld) return NTK_E_SHAPE;
        if (rows->repeat_penalty[b] > 1.0f && rows->n_recent[b] > 0) penalty = true;
    }
    if (penalty && !d_recent) return NTK_E_NULL;
    hipStream_t st = resolve_stream(stream);
    if (penalty)
        hipLaunchKernelGGL(sample_rows_penalty_kernel, dim3(1), dim3(64), 0, st, logits, n_rows, vocab, ld, d_recent, recent_ld, *rows);
    unsigned long long* cand = static_cast<unsigned long long*>(scratch);
    const int cand_ld = chunks * SK_KEEP;
    hipLaunchKernelGGL(sample_rows_stage1, dim3(chunks, n_rows), dim3(SK_THREADS), 0, st, (const float*)logits, vocab, ld, *rows, cand, cand_ld);
    hipLaunchKernelGGL(sample_rows_stage2, dim3(n_rows), dim3(SK_THREADS), 0, st, (const unsigned long long*)cand, cand_ld, chunks, vocab, *rows, d_out,
                       h_mirror);
    return last_launch_status();
}

}  // extern "C"
