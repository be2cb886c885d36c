// sampling.hip -- the reference's token sampler on the device (second half).
//
// Replaces, for temperature > 0 and 0 < top_k <= 64, the per-token host work of the reference's decode loop
// (reference src/inference/engine.cpp:113-119: a blocking 513 KB logits download, then Sampler::apply_repeat_penalty and
// Sampler::sample, reference src/inference/sampler.cpp:30-117, whose std::partial_sort walks all 128 256 candidates).
// Same arithmetic, step for step: the repeat penalty (one application per occurrence in the window, in order), logit /
// temperature, the top-k candidates in descending order, expf(l - max) summed and normalised SEQUENTIALLY in that order by
// one thread (the reference's float summation order), the top-p cut and renormalisation, and the walk of the cumulative
// distribution against a uniform draw.  The draw itself stays on the host (`r`, from the engine's std::mt19937, one per
// token exactly as Sampler::sample consumes it), so the sampled stream is the reference's for the same seed.
//
// Top-k of 128 256 logits: workgroup b sorts its 2048-element chunk in LDS (bitonic, 64-bit keys = orderable value bits :
// inverted index, so ties resolve to the lower token id) and emits its best 64; one workgroup then sorts the
// <= 64 x 63 survivors.  Two launches (+ the penalty), ~0.5 MB of L2-resident reads.
#include "sampling_core.hip.h"

namespace ntk {

// the device code lives in sampling_core.hip.h (shared with the batched sampler, sampling_batch.hip); these are its single-row launches
__global__ void sample_penalty_kernel(float* __restrict__ logits, int n, const int* __restrict__ recent, int n_recent, float penalty) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    sk_penalty(logits, n, recent, n_recent, penalty);
}

__global__ __launch_bounds__(1024) void sample_topk_stage1(const float* __restrict__ logits, int n, float temperature,
                                                           unsigned long long* __restrict__ cand) {
    __shared__ unsigned long long keys[SK_CHUNK];
    sk_stage1(logits, n, temperature, blockIdx.x, cand, keys);
}

__global__ __launch_bounds__(1024) void sample_topk_stage2(const unsigned long long* __restrict__ cand, int n_cand, int top_k,
                                                           float top_p, float r, int* __restrict__ d_out, int* __restrict__ h_mirror) {
    __shared__ unsigned long long keys[SK_MAXCAND];
    sk_stage2(cand, n_cand, top_k, top_p, r, d_out, h_mirror, keys);
}

}  // namespace ntk

extern "C" {

using namespace ntk;

size_t ntk_sample_scratch_bytes(int n) {
    const int chunks = (n + SK_CHUNK - 1) / SK_CHUNK;
    return (size_t)chunks * SK_KEEP * sizeof(unsigned long long) + 256;
}

int ntk_sample_top_k(float* logits, int n, const int* d_recent, int n_recent, float repeat_penalty, float temperature, int top_k,
                     float top_p, float r, int* d_out_token, int* h_mirror, void* scratch, void* stream) {
    if (!logits || !d_out_token || !scratch) return NTK_E_NULL;
    if (n <= 0 || n_recent < 0 || (n_recent > 0 && !d_recent)) return NTK_E_SHAPE;
    if (!(temperature > 0.0f) || top_k <= 0 || top_k > SK_KEEP) return NTK_E_SHAPE;   // greedy: ntk_argmax; wider top-k: host sampler
    const int chunks = (n + SK_CHUNK - 1) / SK_CHUNK;
    if (chunks * SK_KEEP > SK_MAXCAND) return NTK_E_SHAPE;                             // vocabularies beyond 131 072
    hipStream_t st = resolve_stream(stream);
    if (repeat_penalty > 1.0f && n_recent > 0)
        hipLaunchKernelGGL(sample_penalty_kernel, dim3(1), dim3(64), 0, st, logits, n, d_recent, n_recent, repeat_penalty);
    unsigned long long* cand = static_cast<unsigned long long*>(scratch);
    hipLaunchKernelGGL(sample_topk_stage1, dim3(chunks), dim3(1024), 0, st, (const float*)logits, n, temperature, cand);
    hipLaunchKernelGGL(sample_topk_stage2, dim3(1), dim3(1024), 0, st, (const unsigned long long*)cand, chunks * SK_KEEP, top_k < n ? top_k : n,
                       top_p, r, d_out_token, h_mirror);
    return last_launch_status();
}

// the repeat penalty alone (greedy decoding with a penalty: penalty, then ntk_argmax)
int ntk_repeat_penalty(float* logits, int n, const int* d_recent, int n_recent, float repeat_penalty, void* stream) {
    if (!logits || (n_recent > 0 && !d_recent)) return NTK_E_NULL;
    if (n <= 0 || n_recent < 0) return NTK_E_SHAPE;
    if (repeat_penalty > 1.0f && n_recent > 0)
        hipLaunchKernelGGL(sample_penalty_kernel, dim3(1), dim3(64), 0, resolve_stream(stream), logits, n, d_recent, n_recent, repeat_penalty);
    return last_launch_status();
}

}  // extern "C"
