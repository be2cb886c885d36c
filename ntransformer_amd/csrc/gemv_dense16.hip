// gemv_dense16.hip -- fused decode GEMV over unquantised 16-bit weights (IEEE half, bfloat16) on gfx950 (CDNA4, wave64).
//
// The 16-bit side of ntk_gemv_fused (gemv.hip): the same four forms the quantised kernel has -- plain, RMSNorm prologue, residual epilogue, SiLU(gate) x up
// over up to three row segments of ONE dtype sharing x -- so that an F16 / BF16 model's layer is the five launches a quantised one is.  The reference has
// only gemv_f16_kernel (reference src/cuda/gemm.cu:476-560: one row per warp, x re-read from global memory per row) and no bfloat16 at all.
//
// Arithmetic: a weight widens EXACTLY (half -> float: v_cvt_f32_f16; bfloat16 -> float: its bits are the float's high half), products and sums are
// F32 FMAs.  Only the order of summation differs from the oracle's F32 GEMV over the widened weights.
//
// Shape of the kernel:
//   * rows are plain arrays of 16-bit words, so nothing has to be realigned: a lane streams whole 16-byte pieces (8 weights) of a row straight into
//     registers, non-temporal, coalesced (a wave instruction = 1 KiB of one row).  No weight byte passes through LDS;
//   * a wave works on R rows at a time and U pieces of each per step, R x U = 8 independent 16-byte requests per lane in flight (8 KiB per wave);
//   * x -- after the optional RMSNorm, applied by the thread that loaded the element -- is written ONCE per workgroup into LDS as two planes (floats
//     0..3 / 4..7 of every group of 8 columns: a lane's two ds_read_b128 per piece are then conflict-free) and feeds all R rows of a step;
//   * R is chosen per launch (4, 2, 1) so that a launch of few rows (Wo: 4096) still has a workgroup for every CU.
// Shapes: in_features a multiple of 8, W / x / norm_w 16-byte aligned; anything else is NTK_E_ALIGN -- nothing launched, y untouched -- and the caller
// runs the 1:1 sequence (ntk_rmsnorm, ntk_gemv, ntk_add), whose dense kernel has a scalar path.
#include "common.hip.h"
#include <algorithm>

namespace ntk {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr int D16_THREADS = 512;          // 8 waves share one x image
constexpr int D16_MAX_IN = 32768;         // the x image: 128 KiB of the CU's 160
constexpr int D16_MAX_WG = 512;           // two workgroups per CU at most; waves walk their tasks

struct Dense16Params {
    const uint8_t* W[3];
    float* y[3];
    int rows[3];
    int nseg;
    int total;            // row items of the launch (silu_pair: 2 x rows, gate and up rows alternating)
    const float* x;
    int in;
    const float* norm_w;
    float eps;
    const float* resid;
    int silu_pair;
};

template <bool BF> __device__ __forceinline__ float widen_lo(uint32_t w) {
    if constexpr (BF) return __uint_as_float(w << 16); else return h2f((uint16_t)(w & 0xFFFFu));
}
template <bool BF> __device__ __forceinline__ float widen_hi(uint32_t w) {
    if constexpr (BF) return __uint_as_float(w & 0xFFFF0000u); else return h2f((uint16_t)(w >> 16));
}
// acc += the 8 weights of one 16-byte piece . their 8 activations
template <bool BF> __device__ __forceinline__ float dot8(const u32x4 w, const float4 xa, const float4 xb, float acc) {
    acc = fmaf(widen_lo<BF>(w.x), xa.x, acc); acc = fmaf(widen_hi<BF>(w.x), xa.y, acc);
    acc = fmaf(widen_lo<BF>(w.y), xa.z, acc); acc = fmaf(widen_hi<BF>(w.y), xa.w, acc);
    acc = fmaf(widen_lo<BF>(w.z), xb.x, acc); acc = fmaf(widen_hi<BF>(w.z), xb.y, acc);
    acc = fmaf(widen_lo<BF>(w.w), xb.z, acc); acc = fmaf(widen_hi<BF>(w.w), xb.w, acc);
    return acc;
}

// Dynamic LDS: [plane A: in / 2 floats][plane B: in / 2 floats][16 floats reduction scratch]
template <bool BF, bool NORM, int R>
__global__ __launch_bounds__(D16_THREADS) void gemv_dense16_kernel(const Dense16Params p) {
    constexpr int U = 8 / R;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nv = p.in >> 3;                                   // 16-byte pieces per row
    float* const planeA = reinterpret_cast<float*>(smem);
    float* const planeB = planeA + 4 * nv;
    float* const red = planeB + 4 * nv;

    // ---- prologue: x (x * rms_inv * w, the reference's association, rmsnorm.cu:60-68) into the two planes, once per workgroup ----
    {
        const int nq = p.in >> 2;                               // float4s of x
        float rms_inv = 1.0f;
        if constexpr (NORM) {
            float ssq = 0.0f;
            for (int f = tid; f < nq; f += D16_THREADS) {
                const float4 v = *reinterpret_cast<const float4*>(p.x + 4 * f);
                ssq = fmaf(v.x, v.x, ssq); ssq = fmaf(v.y, v.y, ssq); ssq = fmaf(v.z, v.z, ssq); ssq = fmaf(v.w, v.w, ssq);
            }
            ssq = wave_sum(ssq);
            if (lane == 0) red[wave] = ssq;
            __syncthreads();
            float tot = 0.0f;
            for (int w = 0; w < D16_THREADS / 64; ++w) tot += red[w];   // fixed order: the same bits in every workgroup
            rms_inv = 1.0f / sqrtf(tot / (float)p.in + p.eps);
        }
        for (int f = tid; f < nq; f += D16_THREADS) {
            float4 v = *reinterpret_cast<const float4*>(p.x + 4 * f);
            if constexpr (NORM) {
                const float4 w = *reinterpret_cast<const float4*>(p.norm_w + 4 * f);
                v.x = v.x * rms_inv * w.x; v.y = v.y * rms_inv * w.y; v.z = v.z * rms_inv * w.z; v.w = v.w * rms_inv * w.w;
            }
            *reinterpret_cast<float4*>(((f & 1) ? planeB : planeA) + 4 * (f >> 1)) = v;
        }
        __syncthreads();
    }

    // ---- rows: task t = row items [t R, t R + R); the waves of the launch walk the tasks.  Items past the end repeat the last one (not stored). ----
    const int ntasks = (p.total + R - 1) / R;
    const int nwaves = (int)gridDim.x * (D16_THREADS / 64);
    const int nit = (nv + 64 * U - 1) / (64 * U);               // steps per row: uniform
    for (int task = (int)blockIdx.x * (D16_THREADS / 64) + wave; task < ntasks; task += nwaves) {
        const uint8_t* wp[R];
        float* yp[R];
        bool seg0[R];
#pragma unroll
        for (int j = 0; j < R; ++j) {                           // item -> (segment, row): wave-uniform
            const int q = min(task * R + j, p.total - 1);
            int seg = 0, row = q;
            if (p.silu_pair) { seg = q & 1; row = q >> 1; }
            else if (p.nseg > 1 && row >= p.rows[0]) {
                row -= p.rows[0]; seg = 1;
                if (p.nseg > 2 && row >= p.rows[1]) { row -= p.rows[1]; seg = 2; }
            }
            wp[j] = p.W[seg] + (size_t)row * ((size_t)p.in * 2);
            yp[j] = p.y[seg] + row;
            seg0[j] = seg == 0;
        }
        float acc[R];
#pragma unroll
        for (int j = 0; j < R; ++j) acc[j] = 0.0f;
        for (int it = 0; it < nit; ++it) {
            u32x4 w[R][U];
            int pc[U];
#pragma unroll
            for (int u = 0; u < U; ++u) pc[u] = min((it * U + u) * 64 + lane, nv - 1);   // pieces past the row's end re-read its last one
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int j = 0; j < R; ++j)
                    w[j][u] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(wp[j]) + pc[u]);
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const bool have = (it * U + u) * 64 + lane < nv;
                float4 xa = *reinterpret_cast<const float4*>(planeA + 4 * pc[u]);
                float4 xb = *reinterpret_cast<const float4*>(planeB + 4 * pc[u]);
                if (!have) { xa = float4{0.0f, 0.0f, 0.0f, 0.0f}; xb = xa; }             // ... against zeros
#pragma unroll
                for (int j = 0; j < R; ++j) acc[j] = dot8<BF>(w[j][u], xa, xb, acc[j]);
            }
        }
        float tot[R];
#pragma unroll
        for (int j = 0; j < R; ++j) tot[j] = wave_sum(acc[j]);
        if (p.silu_pair) {                                      // items (2k, 2k + 1) = (gate, up) of row k; R is even
#pragma unroll
            for (int j = 0; j < R; j += 2)
                if (lane == j && task * R + j + 1 < p.total) *yp[j] = tot[j] / (1.0f + expf(-tot[j])) * tot[j + 1];   // reference gemm.cu:719-724
        } else {
#pragma unroll
            for (int j = 0; j < R; ++j)
                if (lane == j && task * R + j < p.total) {
                    float v = tot[j];
                    if (p.resid != nullptr && seg0[j]) v = p.resid[yp[j] - p.y[0]] + v;   // reference elementwise.cu:23-32; resid may be y
                    *yp[j] = v;
                }
        }
    }
}

template <bool BF, bool NORM>
static int launch_dense16(const Dense16Params& p, hipStream_t st) {
    // rows per wave step: as many as still leave one workgroup (8 waves) per CU
    const int R = p.total >= 256 * 8 * 4 ? 4 : (p.total >= 256 * 8 * 2 || p.silu_pair) ? 2 : 1;
    const int ntasks = (p.total + R - 1) / R;
    const int grid = std::max(1, std::min((ntasks + D16_THREADS / 64 - 1) / (D16_THREADS / 64), D16_MAX_WG));
    const size_t lds = (size_t)p.in * 4 + 16 * sizeof(float);
    using Fn = void (*)(const Dense16Params);
    static const Fn table[3] = {gemv_dense16_kernel<BF, NORM, 1>, gemv_dense16_kernel<BF, NORM, 2>, gemv_dense16_kernel<BF, NORM, 4>};
    const Fn fn = table[R == 4 ? 2 : R == 2 ? 1 : 0];
    if (lds > 64 * 1024) {
        static const bool raised = [] {
            bool ok = true;
            for (const Fn f : table) ok = ok && hipFuncSetAttribute((const void*)f, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
            return ok;
        }();
        if (!raised) return NTK_E_SHAPE;
    }
    hipLaunchKernelGGL(fn, dim3(grid), dim3(D16_THREADS), lds, st, p);
    return last_launch_status();
}

// the 16-bit side of ntk_gemv_fused: segments of ONE dtype (NTK_DT_F16 / NTK_DT_BF16; the caller has checked that)
int dense16_gemv_fused(const ntk_gemv_seg* segs, int nseg, const float* x, int in, const float* norm_w, float eps, const float* resid, int silu_pair,
                       hipStream_t st) {
    if (in <= 0 || in > D16_MAX_IN) return NTK_E_SHAPE;
    Dense16Params p{};
    long total = 0;
    for (int i = 0; i < nseg; ++i) {
        if (segs[i].rows < 0) return NTK_E_SHAPE;
        if (segs[i].rows > 0 && (!segs[i].W || !segs[i].y)) return NTK_E_NULL;
        if ((size_t)segs[i].rows * (size_t)in * 2 > 0xFFFFFFF0ull) return NTK_E_SHAPE;   // (the limit of the quantised forms)
        p.W[i] = static_cast<const uint8_t*>(segs[i].W);
        p.y[i] = segs[i].y;
        p.rows[i] = segs[i].rows;
        total += segs[i].rows;
    }
    if (silu_pair && (nseg != 2 || segs[0].rows != segs[1].rows || resid)) return NTK_E_SHAPE;
    // whole 16-byte pieces of 16-byte-aligned rows, float4s of x: everything else is the caller's 1:1 sequence
    if (in % 8 != 0 || (reinterpret_cast<uintptr_t>(x) & 15) || (norm_w && (reinterpret_cast<uintptr_t>(norm_w) & 15))) return NTK_E_ALIGN;
    for (int i = 0; i < nseg; ++i)
        if (reinterpret_cast<uintptr_t>(segs[i].W) & 15) return NTK_E_ALIGN;
    if (total == 0) return NTK_OK;
    if (total > 0x3FFFFFFF) return NTK_E_SHAPE;
    if (silu_pair || nseg > 1) {   // empty segments in front would break the kernel's segment walk: drop them (silu_pair has none: total > 0)
        int k = 0;
        for (int i = 0; i < nseg; ++i)
            if (p.rows[i] > 0) { p.W[k] = p.W[i]; p.y[k] = p.y[i]; p.rows[k] = p.rows[i]; ++k; }
        if (resid && segs[0].rows == 0) resid = nullptr;   // (the residual belongs to segment 0)
        nseg = k;
    }
    p.nseg = nseg;
    p.total = (int)total;
    p.x = x; p.in = in; p.norm_w = norm_w; p.eps = eps; p.resid = resid; p.silu_pair = silu_pair;
    const bool bf = segs[0].dtype == NTK_DT_BF16;
    if (bf) return norm_w ? launch_dense16<true, true>(p, st) : launch_dense16<true, false>(p, st);
    return norm_w ? launch_dense16<false, true>(p, st) : launch_dense16<false, false>(p, st);
}

}  // namespace ntk
