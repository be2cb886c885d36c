// common.hip.h -- shared device helpers for the gfx950 (CDNA4, wave64) kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "../../include/ntk_engine.h"

#define NTK_WAVE 64

#define NTK_HIP_TRY(expr)                                   \
    do {                                                    \
        hipError_t e__ = (expr);                            \
        if (e__ != hipSuccess) return NTK_E_LAUNCH;         \
    } while (0)

// Tuning switches exist in tuning builds only (make tune: -DNTK_TUNE -> libntransformer_hip_tune.so, used by tools/*_bench.py and by the
// tests that force a kernel form); the shipping library has the measured constants and reads no environment variable but NTK_DEVICE.
#define NTK_EXTRA_API extern "C" __attribute__((visibility("default")))   // entry points of tuning / trace builds (not in include/*.h)
#ifdef NTK_TUNE
#include <cstdlib>
#define NTK_TUNE_ENV_INT(name, dflt) ([] { const char* e__ = getenv(name); return e__ ? atoi(e__) : (dflt); }())
#else
#define NTK_TUNE_ENV_INT(name, dflt) (dflt)
#endif

namespace ntk {

hipStream_t resolve_stream(void* s);   // runtime.cpp: NULL -> compute stream
int         last_launch_status();      // hipGetLastError -> NTK_OK / NTK_E_LAUNCH
// gemv.hip: the GEMV over the lane-major repack of Q8_0 (ntk_q8l_pack; gemv_core.hip.h: q8l_layout) behind ntk_gemv_rp_fused (gemv_rp.hip)
int         q8l_gemv_fused(const ntk_gemv_seg* segs, int nseg, const float* x, int in, const float* norm_w, float eps, const float* resid,
                           int silu_pair, hipStream_t st);
// gemv_dense16.hip: the fused decode GEMV over unquantised 16-bit rows (segments of ONE dtype, NTK_DT_F16 or NTK_DT_BF16) behind ntk_gemv_fused (gemv.hip)
int         dense16_gemv_fused(const ntk_gemv_seg* segs, int nseg, const float* x, int in, const float* norm_w, float eps, const float* resid,
                               int silu_pair, hipStream_t st);

// ---- fp16 <-> fp32: v_cvt_f32_f16 / v_cvt_f16_f32 (RNE, denormals preserved: hipcc default mode) ----
__device__ __forceinline__ float h2f(uint16_t bits) {
    _Float16 h;
    __builtin_memcpy(&h, &bits, 2);
    return (float)h;
}
__device__ __forceinline__ uint16_t f2h(float f) {
    _Float16 h = (_Float16)f;
    uint16_t bits;
    __builtin_memcpy(&bits, &h, 2);
    return bits;
}

// ---- the RoPE rotation (reference rotary.cu:56-59): two products and a sum per output, every operation rounded on its own -- no fused
//      multiply-add.  hipcc is free to contract `a * c - b * s` either way round (or not at all) per call site, so two kernels given
//      the same inputs could store cache rows that differ in the last bit; one definition with contraction off makes every kernel of the
//      library -- and the CPU restatement, compiled without FMA -- produce the same bits from the same (a, b, cos, sin). ----
__device__ __forceinline__ void rope_rotate(const float a, const float b, const float c, const float s, float& ra, float& rb) {
#pragma clang fp contract(off)
    ra = a * c - b * s;
    rb = b * c + a * s;
}

// ---- the frequency of rotation pair i: entry i of the DEVICE table when there is one (the engine's, a model's scaling factors folded in), else
//      powf evaluated in double and rounded once: reproduces a correctly-rounded powf (what IEEE libm gives the oracle); a 1-ulp slip in the
//      frequency is a 4e-4 rad phase error at position 4095 ----
__device__ __forceinline__ float rope_freq(const float* __restrict__ inv_freq, const int i, const int head_dim, const float theta) {
    return inv_freq ? inv_freq[i] : 1.0f / (float)pow((double)theta, (double)((2.0f * i) / head_dim));
}

// ---- wave64 reductions on the DPP path (no LDS traffic, ~6 dependent VALU ops instead of six ds_bpermute round
//      trips): quad swaps, half-row and row mirrors leave every lane of a 16-lane row with the row total;
//      row_bcast:15 / row_bcast:31 then chain the four rows, so the wave total lands in lanes 48..63. ----
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_or_zero(float v) {   // lanes outside ROW_MASK (or without a source lane) read 0
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_or_self(float v) {   // ... read their own value
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), CTRL, ROW_MASK, 0xF, false));
}
constexpr int DPP_QUAD_1032 = 0xB1, DPP_QUAD_2301 = 0x4E, DPP_ROW_HALF_MIRROR = 0x141, DPP_ROW_MIRROR = 0x140,
              DPP_ROW_BCAST15 = 0x142, DPP_ROW_BCAST31 = 0x143;

// total in lane 63 only (cheapest form: the caller stores from lane 63)
__device__ __forceinline__ float wave_sum_lane63(float v) {
    v += dpp_or_zero<DPP_QUAD_1032, 0xF>(v);
    v += dpp_or_zero<DPP_QUAD_2301, 0xF>(v);
    v += dpp_or_zero<DPP_ROW_HALF_MIRROR, 0xF>(v);
    v += dpp_or_zero<DPP_ROW_MIRROR, 0xF>(v);
    v += dpp_or_zero<DPP_ROW_BCAST15, 0xA>(v);
    v += dpp_or_zero<DPP_ROW_BCAST31, 0xC>(v);
    return v;
}
// every lane ends with the full result (v_readlane_b32 of lane 63)
__device__ __forceinline__ float wave_sum(float v) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(wave_sum_lane63(v)), 63));
}
__device__ __forceinline__ float wave_max(float v) {
    v = fmaxf(v, dpp_or_self<DPP_QUAD_1032, 0xF>(v));
    v = fmaxf(v, dpp_or_self<DPP_QUAD_2301, 0xF>(v));
    v = fmaxf(v, dpp_or_self<DPP_ROW_HALF_MIRROR, 0xF>(v));
    v = fmaxf(v, dpp_or_self<DPP_ROW_MIRROR, 0xF>(v));
    v = fmaxf(v, dpp_or_self<DPP_ROW_BCAST15, 0xA>(v));
    v = fmaxf(v, dpp_or_self<DPP_ROW_BCAST31, 0xC>(v));
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}

// sum over aligned groups of N consecutive lanes (N = 2..32), result in every lane of the group; DPP up to a
// 16-lane row, one ds_bpermute for the 32-lane step
template <int N>
__device__ __forceinline__ float group_sum(float v) {
    static_assert(N == 1 || N == 2 || N == 4 || N == 8 || N == 16 || N == 32, "group size");
    if constexpr (N >= 2) v += dpp_or_zero<DPP_QUAD_1032, 0xF>(v);
    if constexpr (N >= 4) v += dpp_or_zero<DPP_QUAD_2301, 0xF>(v);
    if constexpr (N >= 8) v += dpp_or_zero<DPP_ROW_HALF_MIRROR, 0xF>(v);
    if constexpr (N >= 16) v += dpp_or_zero<DPP_ROW_MIRROR, 0xF>(v);
    if constexpr (N >= 32) v += __shfl_xor(v, 16, 64);
    return v;
}

// Block-wide sum / max through LDS scratch `red` (>= 16 floats). All threads must call; result to all.
__device__ __forceinline__ float block_sum(float v, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_sum(v);
    __syncthreads();  // protect `red` against a previous use
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = 0.0f;
    for (int i = 0; i < nw; ++i) t += red[i];  // fixed order: deterministic
    return t;
}
__device__ __forceinline__ float block_max(float v, float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
    v = wave_max(v);
    __syncthreads();
    if (lane == 0) red[wave] = v;
    __syncthreads();
    float t = red[0];
    for (int i = 1; i < nw; ++i) t = fmaxf(t, red[i]);
    return t;
}

// ---- byte-granular LDS reads: the staged weight stream keeps GGUF's 2-byte alignment -----------------
// gfx950 does execute ds_read_b32/b128 at any byte address (hipcc emits them for a 2-byte-aligned pointer), but
// measured on MI355X the misaligned wide reads are slower than aligned dwords + v_alignbyte_b32 (Q8_0 GEMVs lost
// 10-14 %), so a block's dwords are assembled from aligned reads.
// N consecutive dwords starting at any even offset (N+1 aligned reads)
template <int N>
__device__ __forceinline__ void lds_read_dwords(uint32_t (&dst)[N], const uint8_t* base, int off) {
    const int a = off & ~3;
    const uint32_t sh = (uint32_t)(off & 3);
    uint32_t w[N + 1];
#pragma unroll
    for (int i = 0; i <= N; ++i) w[i] = *reinterpret_cast<const uint32_t*>(base + a + 4 * i);
#pragma unroll
    for (int i = 0; i < N; ++i) dst[i] = __builtin_amdgcn_alignbyte(w[i + 1], w[i], sh);
}
__device__ __forceinline__ uint16_t lds_u16_at(const uint8_t* base, int off) {
    return *reinterpret_cast<const uint16_t*>(base + off);
}

// byte k (0..3) of a dword as float: unsigned / signed
__device__ __forceinline__ float ub2f(uint32_t w, int k) { return (float)((w >> (8 * k)) & 0xFFu); }
__device__ __forceinline__ float sb2f(uint32_t w, int k) { return (float)(int)(int8_t)(w >> (8 * k)); }

// K-quant 6-bit (scale, min) pair j of the 12 packed bytes held in three dwords (types.h:112-117)
__device__ __forceinline__ void kq_scale_min(uint32_t s0, uint32_t s1, uint32_t s2, int j, float& sc, float& mn) {
    const uint64_t lo = (uint64_t)s0 | ((uint64_t)s1 << 32);  // bytes 0..7
    auto byte = [&](int n) -> uint32_t {
        return n < 8 ? (uint32_t)((lo >> (8 * n)) & 0xFFu) : ((s2 >> (8 * (n - 8))) & 0xFFu);
    };
    uint32_t s, m;
    if (j < 4) {
        s = byte(j) & 63u;
        m = byte(j + 4) & 63u;
    } else {
        s = (byte(j + 4) & 0xFu) | ((byte(j - 4) >> 6) << 4);
        m = (byte(j + 4) >> 4) | ((byte(j) >> 6) << 4);
    }
    sc = (float)s;
    mn = (float)m;
}

}  // namespace ntk
