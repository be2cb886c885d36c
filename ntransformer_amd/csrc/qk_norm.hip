// qk_norm.hip -- the per-head RMSNorm of Q and K of Qwen3-family models (GGUF blk.N.attn_q_norm.weight / attn_k_norm.weight): ONE launch normalises every
// head of the q rows and of the k rows in place, ahead of the rotation.  No reference counterpart: the reference runs Llama models only; the arithmetic
// is that of rmsnorm_kernel (elementwise.hip; reference rmsnorm.cu:60-68) on head_dim values: x * (1 / sqrtf(ssq / head_dim + eps)) * w, ssq by fmaf.
//
// One WAVE per (row, head): the head's head_dim / 64 floats per lane stay in registers between the sum of squares and the scaling, the sum goes through
// wave_sum (DPP, no LDS, no barrier), and the weight vector is read once per wave.  Workgroups of 4 waves = 4 consecutive heads of the row's q | k heads.
// Forms, chosen per buffer (q with wq, k with wk) on the host:
//   head_dim 128, buffer and weight 8-byte aligned:    one float2 per lane (lane l holds elements 2l, 2l + 1)
//   head_dim 256, buffer and weight 16-byte aligned:   one float4 per lane (elements 4l .. 4l + 3)
//   everything else (64, 80, 96 ..., any base):        lane-strided, element i in lane i % 64 -- at head_dim 64 that is one float per lane
// The order of the sum depends on the form alone -- head_dim and alignment -- never on the row count or on which head it is: a row of a T-row launch
// has the bits of its one-row launch.  A latency-level kernel: 40 heads of 128 floats at a decode step, 21 MB read and written at a 1024-token prompt.
#include "common.hip.h"

namespace ntk {

struct QkNormArgs {
    float* x[2];           // q [n_rows][heads[0] * head_dim], k [n_rows][heads[1] * head_dim]
    const float* w[2];     // wq, wk: [head_dim]
    int heads[2];
    int form[2];           // 0 lane-strided, 2 float2 (head_dim 128), 4 float4 (head_dim 256)
    int head_dim;
    float eps;
};

__device__ __forceinline__ float qk_rms_inv(float ssq, int head_dim, float eps) {
    return 1.0f / sqrtf(wave_sum(ssq) / (float)head_dim + eps);
}

// grid (ceil(heads[0] + heads[1], 4), n_rows), 256 threads: wave g of a row takes head g of q, then of k
__global__ __launch_bounds__(256) void qk_norm_kernel(const QkNormArgs a) {
    const int lane = threadIdx.x & 63;
    int g = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));   // (wave-uniform: the branches below are scalar)
    int b = 0;
    if (g >= a.heads[0]) { g -= a.heads[0]; b = 1; if (g >= a.heads[1]) return; }
    const int hd = a.head_dim;
    float* const x = a.x[b] + ((size_t)blockIdx.y * (size_t)a.heads[b] + (size_t)g) * (size_t)hd;
    const float* const w = a.w[b];
    const int form = a.form[b];
    if (form == 2) {
        float2 v = reinterpret_cast<const float2*>(x)[lane];
        const float2 c = reinterpret_cast<const float2*>(w)[lane];
        const float r = qk_rms_inv(fmaf(v.y, v.y, fmaf(v.x, v.x, 0.0f)), hd, a.eps);
        v.x = v.x * r * c.x; v.y = v.y * r * c.y;
        reinterpret_cast<float2*>(x)[lane] = v;
    } else if (form == 4) {
        float4 v = reinterpret_cast<const float4*>(x)[lane];
        const float4 c = reinterpret_cast<const float4*>(w)[lane];
        const float r = qk_rms_inv(fmaf(v.w, v.w, fmaf(v.z, v.z, fmaf(v.y, v.y, fmaf(v.x, v.x, 0.0f)))), hd, a.eps);
        v.x = v.x * r * c.x; v.y = v.y * r * c.y; v.z = v.z * r * c.z; v.w = v.w * r * c.w;
        reinterpret_cast<float4*>(x)[lane] = v;
    } else if (hd <= 256) {   // up to four floats per lane, kept in registers
        float v[4], c[4];
        float ssq = 0.0f;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int i = lane + 64 * j;
            v[j] = i < hd ? x[i] : 0.0f;
            c[j] = i < hd ? w[i] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (lane + 64 * j < hd) ssq = fmaf(v[j], v[j], ssq);
        const float r = qk_rms_inv(ssq, hd, a.eps);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (lane + 64 * j < hd) x[lane + 64 * j] = v[j] * r * c[j];
    } else {   // a head wider than 256: read twice
        float ssq = 0.0f;
        for (int i = lane; i < hd; i += 64) ssq = fmaf(x[i], x[i], ssq);
        const float r = qk_rms_inv(ssq, hd, a.eps);
        for (int i = lane; i < hd; i += 64) x[i] = x[i] * r * w[i];
    }
}

}  // namespace ntk

extern "C" int ntk_qk_norm(float* q, float* k, const float* wq, const float* wk, int n_rows, int n_heads, int n_kv_heads, int head_dim, float eps,
                           void* stream) {
    using namespace ntk;
    if (!q || !k || !wq || !wk) return NTK_E_NULL;
    if (head_dim <= 0 || (head_dim & 1) || n_heads <= 0 || n_kv_heads <= 0 || n_rows < 0) return NTK_E_SHAPE;
    if ((long long)n_heads + n_kv_heads > 0x7FFFFFF0ll) return NTK_E_SHAPE;
    if (n_rows == 0) return NTK_OK;
    QkNormArgs a{{q, k}, {wq, wk}, {n_heads, n_kv_heads}, {0, 0}, head_dim, eps};
    for (int b = 0; b < 2; ++b) {
        const uintptr_t bits = (uintptr_t)a.x[b] | (uintptr_t)a.w[b];   // (a row and a head start at a multiple of head_dim floats: the base decides)
        a.form[b] = head_dim == 128 && bits % 8 == 0 ? 2 : head_dim == 256 && bits % 16 == 0 ? 4 : 0;
    }
    const unsigned groups = (unsigned)(((long long)n_heads + n_kv_heads + 3) / 4);
    hipStream_t st = resolve_stream(stream);
    for (int r0 = 0; r0 < n_rows; r0 += 65535) {   // (grid.y holds 65535 rows: a longer prompt goes out in pieces, each row's bits unchanged)
        const int rows = n_rows - r0 < 65535 ? n_rows - r0 : 65535;
        a.x[0] = q + (size_t)r0 * (size_t)n_heads * (size_t)head_dim;
        a.x[1] = k + (size_t)r0 * (size_t)n_kv_heads * (size_t)head_dim;
        hipLaunchKernelGGL(qk_norm_kernel, dim3(groups, (unsigned)rows), dim3(256), 0, st, a);
    }
    return last_launch_status();
}
