// sampling_core.hip.h -- the device code of the sampler, shared by sampling.hip (one row: ntk_sample_top_k) and sampling_batch.hip (up to 16 rows of a
// batched decode step: ntk_sample_rows_top_k).  The kernels of both files are thin wrappers around these bodies, so a row sampled in a batch goes through
// the same instructions in the same order as a row sampled alone (attention_decode.hip.h does the same for the attention kernels).
//
// The arithmetic is the reference's (reference src/inference/sampler.cpp:30-117), step for step: the repeat penalty (one application per occurrence in
// the window, in order), logit / temperature, the top-k candidates in descending order, expf(l - max) summed and normalised SEQUENTIALLY in that order
// by one thread (the reference's float summation order), the top-p cut and renormalisation, and the walk of the cumulative distribution against a
// uniform draw the host took from its std::mt19937.
#pragma once
#include "common.hip.h"
#include <cfloat>

namespace ntk {

constexpr int SK_CHUNK = 2048;    // logits per first-stage workgroup
constexpr int SK_KEEP = 64;       // survivors per chunk = the largest supported top_k
constexpr int SK_MAXCAND = 4096;  // second stage sorts up to this many survivors (64 chunks -> vocabularies up to 131 072)
constexpr int SK_THREADS = 1024;  // workgroup size of both stages

__device__ __forceinline__ unsigned long long sk_key(float v, int idx) {   // larger key = larger value, then smaller index
    uint32_t b = __float_as_uint(v);
    b = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
    return ((unsigned long long)b << 32) | (unsigned long long)(0xFFFFFFFFu - (uint32_t)idx);
}
__device__ __forceinline__ float sk_value(unsigned long long k) {
    uint32_t b = (uint32_t)(k >> 32);
    b = (b & 0x80000000u) ? (b & 0x7FFFFFFFu) : ~b;
    return __uint_as_float(b);
}
__device__ __forceinline__ int sk_index(unsigned long long k) { return (int)(0xFFFFFFFFu - (uint32_t)k); }

// the key of a GREEDY row's logit: Sampler::argmax starts at id 0 and moves on l[i] > l[best], so -0 and +0 tie (the lower id wins), a NaN at an id
// above 0 never wins -- it sorts below -inf here, above the padding (0) -- and a NaN at id 0 is never left (nothing compares greater): the largest key
__device__ __forceinline__ unsigned long long sk_key_greedy(float v, int idx) {
    if (v != v) return idx == 0 ? ~0ull : (unsigned long long)(0xFFFFFFFFu - (uint32_t)idx);
    return sk_key(v + 0.0f, idx);
}

// descending bitonic sort of n (power of two) keys in LDS by the whole workgroup
__device__ void sk_sort_desc(unsigned long long* keys, int n) {
    for (int size = 2; size <= n; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            __syncthreads();
            for (int t = threadIdx.x; t < n / 2; t += blockDim.x) {
                const int lo = 2 * t - (t & (stride - 1));      // index with bit `stride` clear
                const int hi = lo + stride;
                const bool desc = (lo & size) == 0;
                const unsigned long long a = keys[lo], b = keys[hi];
                if ((a < b) == desc) { keys[lo] = b; keys[hi] = a; }
            }
        }
    }
    __syncthreads();
}

// the largest of the workgroup's keys: `mine` of every thread through keys[0 .. blockDim.x) (a power of two), result in every thread
__device__ unsigned long long sk_max_key(unsigned long long* keys, unsigned long long mine) {
    keys[threadIdx.x] = mine;
    for (int stride = blockDim.x >> 1; stride > 0; stride >>= 1) {
        __syncthreads();
        if ((int)threadIdx.x < stride) {
            const unsigned long long a = keys[threadIdx.x], b = keys[threadIdx.x + stride];
            if (b > a) keys[threadIdx.x] = b;
        }
    }
    __syncthreads();
    return keys[0];
}

// reference sampler.cpp:30-45, ONE thread: the window is walked in order, a token that occurs twice is penalised twice, ids outside the row are skipped
__device__ __forceinline__ void sk_penalty(float* __restrict__ logits, int n, const int* __restrict__ recent, int n_recent, float penalty) {
    for (int i = 0; i < n_recent; ++i) {
        const int t = recent[i];
        if (t < 0 || t >= n) continue;
        const float v = logits[t];
        logits[t] = v > 0.0f ? v / penalty : v * penalty;
    }
}

// stage 1, one workgroup per chunk of SK_CHUNK logits: the chunk's SK_KEEP best {logit / temperature, id} to cand[chunk * SK_KEEP ..], descending.
// keys: SK_CHUNK keys of LDS
__device__ __forceinline__ void sk_stage1(const float* __restrict__ logits, int n, float temperature, int chunk, unsigned long long* __restrict__ cand,
                                          unsigned long long* keys) {
    const int base = chunk * SK_CHUNK;
    for (int i = threadIdx.x; i < SK_CHUNK; i += blockDim.x) {
        const int idx = base + i;
        // candidates_[i] = {logits[i] / temperature, i}  (sampler.cpp:56-58); padding sorts last
        keys[i] = idx < n ? sk_key(logits[idx] / temperature, idx) : 0ull;
    }
    sk_sort_desc(keys, SK_CHUNK);
    for (int i = threadIdx.x; i < SK_KEEP; i += blockDim.x) cand[(size_t)chunk * SK_KEEP + i] = keys[i];
}

// stage 1 of a greedy row: the chunk's first maximum alone, to cand[chunk * SK_KEEP] (no division).  keys: blockDim.x keys of LDS
__device__ __forceinline__ void sk_stage1_greedy(const float* __restrict__ logits, int n, int chunk, unsigned long long* __restrict__ cand,
                                                 unsigned long long* keys) {
    const int base = chunk * SK_CHUNK;
    unsigned long long best = 0ull;
    for (int i = threadIdx.x; i < SK_CHUNK; i += blockDim.x) {
        const int idx = base + i;
        const unsigned long long k = idx < n ? sk_key_greedy(logits[idx], idx) : 0ull;
        if (k > best) best = k;
    }
    best = sk_max_key(keys, best);
    if (threadIdx.x == 0) cand[(size_t)chunk * SK_KEEP] = best;
}

// stage 2, one workgroup: the n_cand survivors sorted, then sampler.cpp:73-116 on the k best by one thread.  keys: SK_MAXCAND keys of LDS
__device__ __forceinline__ void sk_stage2(const unsigned long long* __restrict__ cand, int n_cand, int top_k, float top_p, float r,
                                          int* __restrict__ d_out, int* __restrict__ h_mirror, unsigned long long* keys) {
    int npad = 64;
    while (npad < n_cand) npad <<= 1;
    for (int i = threadIdx.x; i < npad; i += blockDim.x) keys[i] = i < n_cand ? cand[i] : 0ull;
    sk_sort_desc(keys, npad);
    if (threadIdx.x != 0) return;
    // one thread, the reference's order of float operations
    int k = top_k;
    while (k > 0 && keys[k - 1] == 0ull) --k;   // vocabulary smaller than top_k
    float p[SK_KEEP];
    const float mx = sk_value(keys[0]);
    float sum = 0.0f;
    for (int i = 0; i < k; ++i) {
        // expf correctly rounded (evaluated in double, rounded once): what the host's libm returns for the reference
        p[i] = (float)exp((double)(sk_value(keys[i]) - mx));
        sum += p[i];
    }
    for (int i = 0; i < k; ++i) p[i] /= sum;
    if (top_p < 1.0f && top_p > 0.0f) {
        float cum = 0.0f;
        int cutoff = k;
        for (int i = 0; i < k; ++i) {
            cum += p[i];
            if (cum >= top_p) { cutoff = i + 1; break; }
        }
        k = cutoff;
        sum = 0.0f;
        for (int i = 0; i < k; ++i) sum += p[i];
        for (int i = 0; i < k; ++i) p[i] /= sum;
    }
    int pick = sk_index(keys[k - 1]);   // fallback (sampler.cpp:115)
    float cum = 0.0f;
    for (int i = 0; i < k; ++i) {
        cum += p[i];
        if (r <= cum) { pick = sk_index(keys[i]); break; }
    }
    *d_out = pick;
    if (h_mirror) *h_mirror = pick;
}

// stage 2 of a greedy row: the first maximum over the chunks' maxima (cand[c * SK_KEEP], c < chunks).  keys: blockDim.x keys of LDS
__device__ __forceinline__ void sk_stage2_greedy(const unsigned long long* __restrict__ cand, int chunks, int* __restrict__ d_out,
                                                 int* __restrict__ h_mirror, unsigned long long* keys) {
    unsigned long long best = 0ull;
    for (int c = threadIdx.x; c < chunks; c += blockDim.x) {
        const unsigned long long k = cand[(size_t)c * SK_KEEP];
        if (k > best) best = k;
    }
    best = sk_max_key(keys, best);
    if (threadIdx.x != 0) return;
    const int pick = sk_index(best);
    *d_out = pick;
    if (h_mirror) *h_mirror = pick;
}

}  // namespace ntk
