// gemm_dense16.hip -- batched prompt projections over unquantised 16-bit weights (IEEE half, bfloat16) on the 16-bit matrix cores of gfx950 (CDNA4, wave64).
//
// Y[T, rows] = X[T, in] . W^T (+ resid) for W stored as raw F16 or BF16 rows, up to 1024 tokens per pass over W and up to three matrices of one dtype
// sharing X (Q | K | V, gate | up).  It takes over from the F32-MFMA form (gemm_prefill.hip), which widens every weight and runs at the F32 matrix rate,
// one sixteenth of the 16-bit one.
//
// Arithmetic -- the weights go to the matrix cores AS THEY LIE IN MEMORY, no conversion instruction on their path; products exact, accumulation F32:
//   * F16 matrices (v_mfma_f32_16x16x32_f16): the activations are the FP16 GEMM's own operand planes (gemm_f16.hip: x scaled by the token's power of two s
//     and split into two FP16 pieces, |x s - h1 - h2| <= 2^-23 |x s|; 1 / s multiplies the finished sum) -- written by ntk_gemm_prepare_x or by the
//     producers' fused split, so reuse_x and the engine's plane bookkeeping serve these matrices unchanged;
//   * BF16 matrices (v_mfma_f32_16x16x32_bf16): a bfloat16 has F32's exponent range, so there is no token scale; x is split into THREE bfloat16 pieces
//     p1 = rn(x), p2 = rn(x - p1), p3 = rn(x - p1 - p2) (rn: to nearest even, a finite x never rounded to infinity) -- both differences are exact in F32 and
//     p1 + p2 + p3 == x for every x whose last bit is no smaller than the smallest bfloat16 subnormal (2^-133).  Narrowing the weights to half instead would
//     lose range (8 exponent bits against 5);
//   * all pieces of a token go into the same F32 accumulator, step by step, pieces in order.  A token's sums do not depend on the other tokens, on the
//     token count, on the tile height or on how many matrices share the launch: the same bits in every form (ntk_gemm_desc.full_form has nothing to choose).
//
// Decomposition: workgroup = 4 waves = 64 RT rows (RT = 4, 2, 1 by the plan: gemm_dense16_plan.h) x one 64-token chunk; a wave owns 16 RT rows and all of
// the chunk's 1, 2 or 4 token blocks.  Per 32-column step a lane loads its weight fragments straight from global memory into registers -- BF16: the 16
// bytes at columns 8 g of row i, the matrix instruction's own order; F16: the two 8-byte halves {4 g .. 4 g + 3, 16 + 4 g .. 16 + 4 g + 3} the FP16 planes
// are ordered by -- one step ahead of their use, and the workgroup copies the step's plane record (1 KiB per plane and token block, lane-contiguous:
// conflict-free ds_write_b128 / ds_read_b128) into the other half of a two-record LDS ring, one barrier per step.  A weight fragment feeds
// planes x token blocks matrix instructions, a plane fragment RT of them: at RT = 4 and 64 tokens a wave issues 32 (F16) / 48 (BF16) matrix instructions
// per step against 4 weight fragments loaded and 8 (12) plane fragments read from LDS.  Everything is compiler-scheduled C++: no inline assembly, hence no hand-kept wait states.
#include "common.hip.h"
#include <algorithm>
#include "gemm_dense16_plan.h"

namespace ntk {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

// ---- bfloat16 pieces -------------------------------------------------------------------------------------------------------------------------
// to nearest even on the bit pattern (uniform over normals and subnormals); a finite x that would round to infinity keeps the largest finite
// bfloat16 -- the remainder then goes to the next piece like any other; Inf / NaN stay what they are (a NaN keeps a mantissa bit)
__device__ __forceinline__ uint32_t bf16_rn(float x) {
    const uint32_t u = __float_as_uint(x);
    if ((u & 0x7F800000u) == 0x7F800000u) return (u >> 16) | ((u & 0x007FFFFFu) ? 0x40u : 0u);
    uint32_t r = (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
    if ((r & 0x7F80u) == 0x7F80u) r -= 1;
    return r;
}
__device__ __forceinline__ float bf16_widen(uint32_t b) { return __uint_as_float(b << 16); }

// ---- pre-pass (BF16): X[T, in] F32 -> three bfloat16 planes in operand order -------------------------------------------------------------------
// grid = (in / 32 steps, 64-token chunks), block = 64 x the token blocks the main kernel reads; tokens behind T are written as zeros
__global__ __launch_bounds__(256) void split_x_bf16_kernel(const float* __restrict__ X, int T, int in, u32x4* __restrict__ planes, size_t chunk_bytes) {
    const int step = blockIdx.x, tb = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int j = lane & 15, g = lane >> 4, t = (int)blockIdx.y * GD_TOK + tb * 16 + j;
    float x[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) x[e] = 0.0f;
    if (t < T) {
        const float* row = X + (size_t)t * in + step * GD_KSTEP + 8 * g;
        const float4 a = *reinterpret_cast<const float4*>(row), b = *reinterpret_cast<const float4*>(row + 4);
        x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w; x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    }
    uint32_t p[GD_BF16_PLANES][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        p[0][e] = bf16_rn(x[e]);
        const float r1 = x[e] - bf16_widen(p[0][e]);   // exact: at most 16 significant bits
        p[1][e] = bf16_rn(r1);
        const float r2 = r1 - bf16_widen(p[1][e]);     // exact: at most 8
        p[2][e] = bf16_rn(r2);
    }
    u32x4* rec = reinterpret_cast<u32x4*>(reinterpret_cast<uint8_t*>(planes) + (size_t)blockIdx.y * chunk_bytes) + (size_t)step * (GD_BF16_PLANES * 4 * 64);
#pragma unroll
    for (int k = 0; k < GD_BF16_PLANES; ++k)
        rec[(k * 4 + tb) * 64 + lane] = u32x4{p[k][0] | (p[k][1] << 16), p[k][2] | (p[k][3] << 16), p[k][4] | (p[k][5] << 16), p[k][6] | (p[k][7] << 16)};
}

// ---- main kernel -------------------------------------------------------------------------------------------------------------------------------
struct Dense16GemmSeg { const uint8_t* W; float* Y; int rows, tile0; };
struct Dense16GemmParams {
    Dense16GemmSeg seg[GB_MAX_SEG];
    int nseg, T, in, steps, tiles, chunks;
    const uint8_t* planes;      // the pass's operand planes (workspace)
    size_t chunk_bytes;
    const float* inv;           // F16: the tokens' 1 / s; BF16: unused
    const float* resid;         // optional, one matrix only, may alias Y
};

template <bool BF> struct WFrag;
template <> struct WFrag<false> {   // F16: columns {4 g .. 4 g + 3} and {16 + 4 g .. 16 + 4 g + 3} of the step, the FP16 planes' order
    u32x2 lo, hi;
    __device__ __forceinline__ void load(const uint8_t* p) { lo = *reinterpret_cast<const u32x2*>(p); hi = *reinterpret_cast<const u32x2*>(p + 32); }
    __device__ __forceinline__ f32x4 mfma(const u32x4 b, const f32x4 c) const {
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, u32x4{lo.x, lo.y, hi.x, hi.y}), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
    }
    static constexpr int LANE_BYTES = 8;
};
template <> struct WFrag<true> {    // BF16: columns 8 g .. 8 g + 7
    u32x4 w;
    __device__ __forceinline__ void load(const uint8_t* p) { w = *reinterpret_cast<const u32x4*>(p); }
    __device__ __forceinline__ f32x4 mfma(const u32x4 b, const f32x4 c) const {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
    }
    static constexpr int LANE_BYTES = 16;
};

template <bool BF, int RT, int NTB>
__global__ __launch_bounds__(64 * GD_WAVES) void gemm_dense16_kernel(const Dense16GemmParams p) {
    constexpr int P = BF ? GD_BF16_PLANES : GD_F16_PLANES;
    constexpr int REC = P * NTB * 64;                       // 16-byte pieces of a step's record in LDS: [plane][token block][lane]
    constexpr int NLD = (REC + 64 * GD_WAVES - 1) / (64 * GD_WAVES);
    constexpr int STEP_PIECES = P * 4 * 64;                 // ... and in the workspace, which always has four token blocks per plane
    extern __shared__ u32x4 ring[];                         // [2][REC]
    const int tid = (int)threadIdx.x, wave = tid >> 6, lane = tid & 63, j = lane & 15, g = lane >> 4;
    int tile, chunk;
    if (!gd_map(blockIdx.x, p.tiles, p.chunks, tile, chunk)) return;   // (uniform)
    Dense16GemmSeg sg = p.seg[0];
    if (p.nseg > 1 && tile >= p.seg[1].tile0) sg = p.seg[1];
    if (p.nseg > 2 && tile >= p.seg[2].tile0) sg = p.seg[2];
    const int row0 = (tile - sg.tile0) * (64 * RT) + wave * (16 * RT);
    const size_t row_bytes = (size_t)p.in * 2;

    // a row tile that lies behind the matrix reads the matrix's first rows instead (never stored)
    const uint8_t* wp[RT];
#pragma unroll
    for (int r = 0; r < RT; ++r) {
        const int row = row0 + 16 * r < sg.rows ? row0 + 16 * r + j : j;
        wp[r] = sg.W + (size_t)row * row_bytes + g * WFrag<BF>::LANE_BYTES;
    }
    // this thread's pieces of a step record: workspace piece -> ring piece
    const u32x4* src = reinterpret_cast<const u32x4*>(p.planes + (size_t)chunk * p.chunk_bytes);
    int from[NLD], to[NLD];
#pragma unroll
    for (int k = 0; k < NLD; ++k) {
        const int idx = tid + k * 64 * GD_WAVES, rec = idx >> 6;
        to[k] = idx < REC ? idx : -1;
        from[k] = ((rec / NTB) * 4 + rec % NTB) * 64 + (idx & 63);
    }

    f32x4 acc[RT][NTB];
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int b = 0; b < NTB; ++b) acc[r][b] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};

    WFrag<BF> cur[RT], nxt[RT];
    u32x4 pre[NLD];
#pragma unroll
    for (int k = 0; k < NLD; ++k) if (to[k] >= 0) ring[to[k]] = src[from[k]];
#pragma unroll
    for (int r = 0; r < RT; ++r) { cur[r].load(wp[r]); nxt[r] = cur[r]; }
    __syncthreads();

    for (int step = 0; step < p.steps; ++step) {
        const u32x4* rd = ring + (step & 1) * REC;
        const bool more = step + 1 < p.steps;
        if (more) {   // the next step's operands travel while this step's matrix instructions run
#pragma unroll
            for (int k = 0; k < NLD; ++k) if (to[k] >= 0) pre[k] = src[(size_t)(step + 1) * STEP_PIECES + from[k]];
#pragma unroll
            for (int r = 0; r < RT; ++r) nxt[r].load(wp[r] + (size_t)(step + 1) * (GD_KSTEP * 2));
        }
#pragma unroll
        for (int k = 0; k < P; ++k)
#pragma unroll
            for (int b = 0; b < NTB; ++b) {
                const u32x4 x = rd[(k * NTB + b) * 64 + lane];
#pragma unroll
                for (int r = 0; r < RT; ++r) acc[r][b] = cur[r].mfma(x, acc[r][b]);
            }
        if (more) {
            u32x4* wr = ring + ((step + 1) & 1) * REC;
#pragma unroll
            for (int k = 0; k < NLD; ++k) if (to[k] >= 0) wr[to[k]] = pre[k];
        }
        __syncthreads();   // the record just written is complete; the one just read is free
#pragma unroll
        for (int r = 0; r < RT; ++r) cur[r] = nxt[r];
    }

    // the accumulator of lane (j, g) holds rows 4 g .. 4 g + 3 of the tile for token j of the block: one float4 of Y per tile and block
#pragma unroll
    for (int b = 0; b < NTB; ++b) {
        const int tl = chunk * GD_TOK + b * 16 + j;
        if (tl >= p.T) continue;
        float inv = 1.0f;
        if constexpr (!BF) inv = p.inv[tl];
#pragma unroll
        for (int r = 0; r < RT; ++r) {
            const int row = row0 + 16 * r;
            if (row >= sg.rows) continue;
            const size_t at = (size_t)tl * sg.rows + row + 4 * g;
            f32x4 v = acc[r][b];
            if constexpr (!BF) v *= inv;   // (a power of two: exact)
            if (p.resid) v += *reinterpret_cast<const f32x4*>(p.resid + at);
            *reinterpret_cast<f32x4*>(sg.Y + at) = v;
        }
    }
}

template <bool BF, int RT> static void launch_dense16_ntb(const Dense16Plan& plan, const Dense16GemmParams& p, hipStream_t st) {
    const dim3 grid(plan.grid_x), block(plan.block);
    if (plan.ntb == 1) hipLaunchKernelGGL((gemm_dense16_kernel<BF, RT, 1>), grid, block, plan.lds, st, p);
    else if (plan.ntb == 2) hipLaunchKernelGGL((gemm_dense16_kernel<BF, RT, 2>), grid, block, plan.lds, st, p);
    else hipLaunchKernelGGL((gemm_dense16_kernel<BF, RT, 4>), grid, block, plan.lds, st, p);
}
template <bool BF> static void launch_dense16(const Dense16Plan& plan, const Dense16GemmParams& p, hipStream_t st) {
    if (plan.rt == 1) launch_dense16_ntb<BF, 1>(plan, p, st);
    else if (plan.rt == 2) launch_dense16_ntb<BF, 2>(plan, p, st);
    else launch_dense16_ntb<BF, 4>(plan, p, st);
}

}  // namespace ntk

extern "C" {

size_t ntk_gemm_dense16_workspace_bytes(int in_features, int out_features, int dtype) {
    if (in_features <= 0 || out_features < 0 || (dtype != NTK_DT_F16 && dtype != NTK_DT_BF16)) return 0;
    return ntk::gd_workspace_bytes((in_features + 31) / 32 * 32, dtype);
}

int ntk_gemm_dense16(const ntk_gemm_desc* d, void* stream) {
    using namespace ntk;
    if (!d || !d->segs || !d->X || !d->workspace) return NTK_E_NULL;
    const int nseg = d->nseg, in = d->in_features;
    if (nseg < 1 || nseg > GB_MAX_SEG || d->n_tokens < 0 || in <= 0 || (d->resid && nseg != 1) || d->weights_repacked) return NTK_E_SHAPE;
    int rows[GB_MAX_SEG], dtypes[GB_MAX_SEG];
    uintptr_t ptrs[2 * GB_MAX_SEG + 3];
    int nptr = 0;
    for (int i = 0; i < nseg; ++i) {
        if (!d->segs[i].W || !d->segs[i].y) return NTK_E_NULL;
        rows[i] = d->segs[i].rows; dtypes[i] = d->segs[i].dtype;
        ptrs[nptr++] = reinterpret_cast<uintptr_t>(d->segs[i].W); ptrs[nptr++] = reinterpret_cast<uintptr_t>(d->segs[i].y);
    }
    ptrs[nptr++] = reinterpret_cast<uintptr_t>(d->X); ptrs[nptr++] = reinterpret_cast<uintptr_t>(d->resid); ptrs[nptr++] = reinterpret_cast<uintptr_t>(d->workspace);
    // (the plan of the first pass refuses what any pass would: the refusals do not depend on the token count within 1 .. 1024)
    const Dense16Plan first = gemm_dense16_plan(rows, dtypes, nseg, std::max(1, std::min(d->n_tokens, GD_MAX_TOKENS)), in, ptrs, nptr);
    if (first.status != NTK_OK) return first.status;
    if (d->workspace_bytes < first.ws_bytes) return NTK_E_SHAPE;
    if (d->partials) {   // nothing is ever deferred: Y is written, with the residual
        ntk_gemm_partials* pt = d->partials;
        pt->nseg = nseg; pt->n_tokens = d->n_tokens; pt->nsplit = 1;
        for (int i = 0; i < nseg; ++i) { pt->part[i] = nullptr; pt->y[i] = d->segs[i].y; pt->rows[i] = rows[i]; }
    }
    if (d->n_tokens == 0) return NTK_OK;
    hipStream_t st = resolve_stream(stream);
    const bool bf = first.dtype == NTK_DT_BF16;
    uint8_t* wsb = static_cast<uint8_t*>(d->workspace);
    for (int t0 = 0; t0 < d->n_tokens; t0 += GD_MAX_TOKENS) {   // the planes hold one pass (1024 tokens) at a time
        const int T = std::min(GD_MAX_TOKENS, d->n_tokens - t0);
        const Dense16Plan plan = gemm_dense16_plan(rows, dtypes, nseg, T, in);
        const float* X = d->X + (size_t)t0 * in;
        if (!(d->reuse_x && d->n_tokens <= GD_MAX_TOKENS)) {
            if (bf) {
                hipLaunchKernelGGL(split_x_bf16_kernel, dim3(plan.steps, plan.chunks), dim3(64 * plan.ntb), 0, st, X, T, in, reinterpret_cast<u32x4*>(wsb), plan.chunk_bytes);
            } else {   // the FP16 GEMM's planes, by its own public pre-pass (row maximum + split, one launch: row_max is not needed)
                const int rc = ntk_gemm_prepare_x(X, T, in, wsb, stream);
                if (rc != NTK_OK) return rc;
            }
        }
        Dense16GemmParams p{};
        p.nseg = nseg; p.T = T; p.in = in; p.steps = plan.steps; p.tiles = plan.tiles; p.chunks = plan.chunks;
        p.planes = wsb; p.chunk_bytes = plan.chunk_bytes;
        p.inv = reinterpret_cast<const float*>(wsb + gd_inv_offset(in));
        p.resid = d->resid ? d->resid + (size_t)t0 * rows[0] : nullptr;
        for (int i = 0; i < nseg; ++i)
            p.seg[i] = Dense16GemmSeg{static_cast<const uint8_t*>(d->segs[i].W), d->segs[i].y + (size_t)t0 * rows[i], rows[i], plan.seg[i].tile0};
        if (bf) launch_dense16<true>(plan, p, st); else launch_dense16<false>(plan, p, st);
    }
    return last_launch_status();
}

}  // extern "C"
