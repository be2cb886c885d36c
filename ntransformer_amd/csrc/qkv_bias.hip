// qkv_bias.hip -- the Q | K | V projection bias of Qwen2-family models (GGUF blk.N.attn_{q,k,v}.bias): ONE launch adds the three F32 bias vectors to the
// rows of the three projection outputs, in place, ahead of the rotation.  No reference counterpart: the reference runs Llama models only.
//
// Each element is one F32 add -- numpy's float32 sum bit for bit.  A buffer is walked in 16-byte pieces when its base, its bias and its row pitch allow
// them (base and bias 16-byte aligned, the dimension a multiple of 4: every row then starts aligned), element by element otherwise; the choice is per
// buffer.  A latency-level kernel: 4608 floats at a decode step, 18 MB read and written at a 1024-token prompt of a 7B model.
#include "common.hip.h"

namespace ntk {

struct QkvBiasArgs {
    float* x[3];            // q | k | v rows, [n_rows][dim]
    const float* b[3];      // their biases, [dim]; a buffer without one has units = 0
    int dim[3];
    int units[3];           // work items per row: dim / 4 (16-byte pieces) or dim (scalars)
    int vec[3];
};

// grid (n_rows, ceil(units[0] + units[1] + units[2], 256)): thread u of a row takes piece u of q, then of k, then of v
__global__ __launch_bounds__(256) void qkv_bias_kernel(const QkvBiasArgs a) {
    const size_t row = blockIdx.x;
    int u = blockIdx.y * 256 + threadIdx.x;
    int w = 0;
    if (u >= a.units[0]) { u -= a.units[0]; w = 1; if (u >= a.units[1]) { u -= a.units[1]; w = 2; if (u >= a.units[2]) return; } }
    float* const x = a.x[w] + row * (size_t)a.dim[w];
    const float* const b = a.b[w];
    if (a.vec[w]) {
        float4 v = reinterpret_cast<const float4*>(x)[u];
        const float4 c = reinterpret_cast<const float4*>(b)[u];
        v.x += c.x; v.y += c.y; v.z += c.z; v.w += c.w;
        reinterpret_cast<float4*>(x)[u] = v;
    } else {
        x[u] += b[u];
    }
}

}  // namespace ntk

extern "C" int ntk_qkv_bias(float* q, float* k, float* v, const float* bq, const float* bk, const float* bv, int n_rows, int q_dim, int kv_dim, void* stream) {
    using namespace ntk;
    if ((bq && !q) || (bk && !k) || (bv && !v)) return NTK_E_NULL;
    if (n_rows < 0 || q_dim <= 0 || kv_dim <= 0) return NTK_E_SHAPE;
    if (n_rows == 0 || (!bq && !bk && !bv)) return NTK_OK;
    QkvBiasArgs a{{q, k, v}, {bq, bk, bv}, {q_dim, kv_dim, kv_dim}, {0, 0, 0}, {0, 0, 0}};
    long long total = 0;
    for (int w = 0; w < 3; ++w) {
        if (!a.b[w]) continue;
        a.vec[w] = a.dim[w] % 4 == 0 && ((uintptr_t)a.x[w] | (uintptr_t)a.b[w]) % 16 == 0;
        a.units[w] = a.vec[w] ? a.dim[w] / 4 : a.dim[w];
        total += a.units[w];
    }
    const long long blocks = (total + 255) / 256;
    if (blocks > 65535) return NTK_E_SHAPE;   // (16.7 M elements per row: no model is that wide)
    hipLaunchKernelGGL(qkv_bias_kernel, dim3((unsigned)n_rows, (unsigned)blocks), dim3(256), 0, resolve_stream(stream), a);
    return last_launch_status();
}
