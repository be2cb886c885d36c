// logprob.hip -- scoring: per row of F32 logits the log-probability of one target token and the greedy token (ntk_logprob_rows).
//
// No reference counterpart (the reference samples from the last position's logits and never normalises a whole row).  One workgroup of 16 waves
// per row, ONE pass over the row: every lane keeps the online-softmax pair (m, s) -- m the largest logit it has seen, s = sum of expf(x - m) over
// what it has seen -- and the index at which m first occurred, so the same pass yields the first maximum (ntk_argmax's rule: strict >, NaN never
// wins).  m only changes in the first few steps of a lane, so the rescale s *= expf(m_old - m_new) sits in a branch that is almost never taken and
// the steady state is one accurate expf per element.  The row is read in 16-byte pieces from the first 16-byte boundary on (four pieces in flight
// per lane); the up to three floats in front of it and behind the last whole piece are read one by one.  Nothing outside [row, row + vocab) is read.
//
// Order of operations (fixed: the same bits on every launch): lane-sequential over the lane's pieces (the four terms of a piece summed pairwise),
// a butterfly over the 64 lanes, the 16 wave states merged in wave order by thread 0.  Result: (l_t - m) - logf(S).
//   -inf logits add 0 (never expf(-inf - -inf)); a row of -inf only: m = -inf, S = 0 -> (-inf - -inf) = NaN; a NaN logit makes s NaN and with it the
//   row's result (fmaxf drops it from m, so the other rows' arithmetic and this row's top-1 do not see it).
#include "common.hip.h"
#include <cfloat>

namespace ntk {

constexpr int LP_THREADS = 1024;   // 16 waves: one row of 128 256 floats = 32 pieces per lane, 4 in flight
constexpr int LP_WAVES = LP_THREADS / 64;
constexpr int LP_NOIDX = 0x7FFFFFFF;

struct LpState { float m, s; int idx; };

// one element (index i, increasing per lane)
__device__ __forceinline__ void lp_take(LpState& a, float x, int i) {
    if (x > a.m) { a.s *= expf(a.m - x); a.m = x; a.idx = i; }   // (a.m = -inf: expf(-inf) = 0 and s is 0)
    a.s += x == -INFINITY ? 0.0f : expf(x - a.m);
}
// a 16-byte piece, elements i .. i + 3
__device__ __forceinline__ void lp_take4(LpState& a, const float4 v, int i) {
    const float lm = fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w));
    if (lm > a.m) {
        a.s *= expf(a.m - lm);
        a.m = lm;
        a.idx = v.x == lm ? i : v.y == lm ? i + 1 : v.z == lm ? i + 2 : i + 3;
    }
    const float e0 = v.x == -INFINITY ? 0.0f : expf(v.x - a.m), e1 = v.y == -INFINITY ? 0.0f : expf(v.y - a.m);
    const float e2 = v.z == -INFINITY ? 0.0f : expf(v.z - a.m), e3 = v.w == -INFINITY ? 0.0f : expf(v.w - a.m);
    a.s += (e0 + e1) + (e2 + e3);
}
// two states over disjoint index sets.  The two products are rounded on their own and then added (no fused multiply-add, which would round one side's
// product and not the other's): the merge is commutative bit for bit, so both sides of a butterfly step hold the same state afterwards.
__device__ __forceinline__ LpState lp_merge(const LpState a, const LpState b) {
#pragma clang fp contract(off)
    LpState r;
    r.m = fmaxf(a.m, b.m);
    const float fa = a.m == -INFINITY ? 0.0f : expf(a.m - r.m), fb = b.m == -INFINITY ? 0.0f : expf(b.m - r.m);
    r.s = a.s * fa + b.s * fb;
    r.idx = (b.m > a.m || (b.m == a.m && b.idx < a.idx)) ? b.idx : a.idx;
    return r;
}

__global__ __launch_bounds__(LP_THREADS) void logprob_rows_kernel(const float* __restrict__ logits, int vocab, int ld, const int* __restrict__ targets,
                                                                  float* __restrict__ logprob, int* __restrict__ top1) {
    __shared__ LpState red[LP_WAVES];
    const int r = blockIdx.x, tid = threadIdx.x;
    const int target = targets[r];
    if (target < 0 && !top1) {   // skipped row (uniform over the workgroup)
        if (tid == 0) logprob[r] = 0.0f;
        return;
    }
    const float* row = logits + (size_t)r * (size_t)ld;
    // floats up to the first 16-byte boundary, whole pieces, floats behind the last whole piece
    const int head = min(vocab, (int)((4u - (unsigned)((reinterpret_cast<uintptr_t>(row) >> 2) & 3u)) & 3u));
    const int nvec = (vocab - head) >> 2;
    const int tail0 = head + 4 * nvec;
    LpState a{-INFINITY, 0.0f, LP_NOIDX};
    if (tid < head) lp_take(a, row[tid], tid);
    const float4* pieces = reinterpret_cast<const float4*>(row + head);
    const float4 none = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);   // takes no part: never > m, adds 0
    // Every load is UNCONDITIONAL (a guarded one is split by the compiler into four dword loads under exec branches): a piece index past the end is
    // clamped to the last piece -- inside the row -- and what it loaded is replaced by `none` afterwards.
    for (int base = 0; base < nvec; base += 4 * LP_THREADS) {
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) v[u] = pieces[min(base + u * LP_THREADS + tid, nvec - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = base + u * LP_THREADS + tid;
            lp_take4(a, p < nvec ? v[u] : none, head + 4 * p);
        }
    }
    if (tail0 + tid < vocab) lp_take(a, row[tail0 + tid], tail0 + tid);   // (tid < 3; the lane's largest index)
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        LpState o;
        o.m = __shfl_xor(a.m, off, 64); o.s = __shfl_xor(a.s, off, 64); o.idx = __shfl_xor(a.idx, off, 64);
        a = lp_merge(a, o);
    }
    if ((tid & 63) == 0) red[tid >> 6] = a;
    __syncthreads();
    if (tid != 0) return;
    for (int w = 1; w < LP_WAVES; ++w) a = lp_merge(a, red[w]);
    if (top1) top1[r] = a.idx == LP_NOIDX ? 0 : a.idx;   // nothing but -inf / NaN: 0, as ntk_argmax
    if (target < 0) { logprob[r] = 0.0f; return; }
    const float lt = row[min(target, vocab - 1)];   // (the caller validates targets; clamped so that the row is never left)
    logprob[r] = (lt - a.m) - logf(a.s);
}

}  // namespace ntk

extern "C" int ntk_logprob_rows(const float* logits, int n_rows, int vocab, int ld, const int* targets, float* logprob, int* top1, void* stream) {
    if (!logits || !targets || !logprob) return NTK_E_NULL;
    if (n_rows < 0 || vocab <= 0 || ld < vocab) return NTK_E_SHAPE;
    if (reinterpret_cast<uintptr_t>(logits) & 3) return NTK_E_ALIGN;
    if (n_rows == 0) return NTK_OK;
    hipLaunchKernelGGL(ntk::logprob_rows_kernel, dim3((unsigned)n_rows), dim3(ntk::LP_THREADS), 0, ntk::resolve_stream(stream), logits, vocab, ld, targets,
                       logprob, top1);
    return ntk::last_launch_status();
}
