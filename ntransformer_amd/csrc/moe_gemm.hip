// moe_gemm.hip -- the routed expert FFN of a PROMPT pass on the matrix cores: the grouped form of gemm_prefill.hip's F32-MFMA GEMM over raw GGUF blocks.
// No reference counterpart (the reference runs dense Llama layers only).  Two entry points with the arguments, work list and buffer layouts of moe.hip's
// ntk_moe_gate_up / ntk_moe_down, so the engine (and a test) swaps one form for the other on the same buffers:
//
//   ntk_moe_gemm_gate_up  act[p] = SiLU(Wg[e] . xn[t]) x (Wu[e] . xn[t]): two launches of the kernel below -- the gate products go to act, the up launch's
//                         epilogue reads them back and writes g / (1 + expf(-g)) * u over them (each tensor its own type; no scratch: the size is 0).
//   ntk_moe_gemm_down     part[p] = Wd[e] . act[p] by the same kernel, then the GEMV form's own combine y[t] = resid[t] + sum_k fmaf(w[p], part[p], s),
//                         k ascending, one thread per output element.
//
// Arithmetic: weights dequantised to F32 by gemm_deq.hip.h's Deq<DT> (what gemm_prefill.hip feeds the same instruction), F32 activations unrounded,
// v_mfma_f32_16x16x4_f32, F32 accumulation.
//
// Decomposition (gfx950, wave64).  A TILE is up to 16 consecutive entries of one expert's range of the work list (moe_tiles.h): the MFMA's 16 columns.
// Grid (row block, tile): blockIdx.y < ceil(T K / 16) + E is a tile NUMBER; the workgroup finds its (expert, first entry) itself -- one thread per expert
// reads the clamped range, a prefix sum over the tile counts, the thread whose interval holds the number publishes it -- and exits if there is no such
// tile.  No host round trip, no atomics, no launch parameter depends on the routing.  A workgroup is 8 waves; wave w owns output rows 16 w .. 16 w + 15 of
// the block's 128 and walks the WHOLE row length in steps of 256 columns, so a row's sum never crosses a wave: rows of any length (Mixtral's down
// projection: 14336 columns) accumulate in the wave's registers in one fixed order.  Per step the workgroup stages the tile's activations once
// (16 gathered rows x 256 columns, zeros for columns without an entry) and every wave its own 16 weight rows' bytes into LDS -- both requested one step
// ahead, in registers -- then lane (r = lane % 16, g = lane / 16) decodes the 8 weights of row r, columns 32 s + 8 g .. + 7 of each sub-block s as the
// A operand and reads the matching 8 activations of column lane % 16 as B.
//
// Why a pair's bits are its own: a column of the MFMA never meets another column, the order of the products inside a column is fixed by (step, s, j)
// alone, and the weights do not know the column.  So a pair's results do not depend on T, on the pairs it shares a tile with, on the tile or the column
// it falls into, or on the launch; a NaN in one token's row stays in that token's pairs.
#include "common.hip.h"
#include "gemm_deq.hip.h"
#include "moe_tiles.h"

namespace ntk {

constexpr int MG_WAVES = 8;                 // waves per workgroup, each with a 16-row output tile of its own
constexpr int MG_ROWS = 16 * MG_WAVES;      // output rows per workgroup
constexpr int MG_STEP = 256;                // columns per step (a K-quant block; eight Q8_0 blocks)
constexpr int MG_XPITCH = MG_STEP + 4;      // floats per staged activation row (+4: the 16 rows start on different banks)
constexpr int MG_XQ = 16 * (MG_STEP / 4) / (64 * MG_WAVES);   // float4 of the activation tile per thread
constexpr int kMgMaxE = 256, kMgMaxK = 16, kMgMaxT = 1024;    // moe.hip's limits

template <int DT> struct MgGeom {
    static constexpr int SB = GFmt<DT>::SB;                      // bytes of a row inside one step
    static constexpr int PIECES = (SB + 15 + 15) / 16;           // 16-byte pieces that cover them at any alignment
    static constexpr int PITCH = 16 * ((PIECES + 1) | 1);        // LDS bytes per staged row: room for the decoders' dword behind the last byte, an odd
                                                                 // count of 16-byte units so that the 16 rows start on different banks
    static constexpr int NLD = (16 * PIECES + 63) / 64;          // 16-byte loads per lane that fetch a wave's 16 rows
};

struct MoeGemmArgs {
    const uint8_t* W;       // [E][M][row_bytes]
    const float* B;         // activation rows [.][in]: row pairs[i] / bdiv
    float* out;             // [n_pairs][M]
    const int* offsets; const int* pairs;
    size_t expert_bytes;
    unsigned row_bytes;
    int M, in, bdiv, n_pairs, E;
};

// EPI: out holds the gate products; write SiLU(gate) x this launch's products over them
template <int DT, bool FULL, bool EPI>
__global__ __launch_bounds__(64 * MG_WAVES) void moe_gemm_kernel(const MoeGemmArgs a) {
    using Gm = MgGeom<DT>;
    __shared__ __attribute__((aligned(16))) uint8_t s_img[MG_WAVES * 16 * Gm::PITCH];
    __shared__ __attribute__((aligned(16))) float s_x[16 * MG_XPITCH];
    __shared__ int s_wtot[MG_WAVES], s_tile[3], s_pair[16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    // ---- which tile is blockIdx.y?  thread e: expert e's tile count, an inclusive scan in the wave, the waves' totals through LDS (moe_tiles.h: moe_tile_find)
    int beg = 0, end = 0;
    const int n = tid < a.E ? moe_range_tiles(a.offsets, tid, a.n_pairs, beg, end) : 0;
    int inc = n;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int v = __shfl_up(inc, off, 64);
        if (lane >= off) inc += v;
    }
    if (lane == 63) s_wtot[wave] = inc;
    if (tid == 0) s_tile[0] = -1;
    __syncthreads();
    int start = inc - n;
    for (int w = 0; w < wave; ++w) start += s_wtot[w];
    const int tile = (int)blockIdx.y;
    if (n > 0 && tile >= start && tile < start + n) { s_tile[0] = tid; s_tile[1] = beg + MOE_TILE * (tile - start); s_tile[2] = end; }
    __syncthreads();
    const int expert = s_tile[0];
    if (expert < 0) return;   // past the last tile (the whole workgroup)
    if (tid < MOE_TILE) {     // the tile's pair indices; -1: no entry in this column, or an index outside [0, n_pairs): nothing is read or written for it
        const int at = s_tile[1] + tid;
        int p = at < s_tile[2] ? a.pairs[at] : -1;
        if (p < 0 || p >= a.n_pairs) p = -1;
        s_pair[tid] = p;
    }
    __syncthreads();

    const int row0 = (int)blockIdx.x * MG_ROWS + 16 * wave;
    const bool live = row0 < a.M;   // wave-uniform; a wave without rows still stages activations and meets the barriers
    const uint8_t* const We = a.W + (size_t)expert * a.expert_bytes;
    const int r = lane & 15, g = lane >> 4;
    const uint8_t* const my_row = We + (size_t)min(row0 + r, a.M - 1) * a.row_bytes;   // the row this lane decodes (a ragged last tile re-reads the last row)
    const int nsteps = (a.in + MG_STEP - 1) / MG_STEP;

    u32x4 wpf[Gm::NLD];
    float4 xpf[MG_XQ];
    auto issue = [&](int step) {
        const unsigned cbyte = (unsigned)step * Gm::SB;
        const unsigned clen = min((unsigned)Gm::SB, a.row_bytes - cbyte);
        if (live) {
#pragma unroll
            for (int q = 0; q < Gm::NLD; ++q) {
                const int idx = min(lane + 64 * q, 16 * Gm::PIECES - 1), row = idx / Gm::PIECES, piece = idx % Gm::PIECES;
                const uintptr_t p = (uintptr_t)(We + (size_t)min(row0 + row, a.M - 1) * a.row_bytes + cbyte);
                const unsigned last = ((unsigned)(p & 15u) + clen - 1u) >> 4;   // the piece that holds the row's last byte of this step
                wpf[q] = *reinterpret_cast<const u32x4*>((p & ~(uintptr_t)15) + 16u * min((unsigned)piece, last));
            }
        }
#pragma unroll
        for (int q = 0; q < MG_XQ; ++q) {
            const int idx = tid + 64 * MG_WAVES * q, tok = idx / (MG_STEP / 4), col = step * MG_STEP + 4 * (idx % (MG_STEP / 4));
            const int p = s_pair[tok];
            const bool have = p >= 0 && col < a.in;
            xpf[q] = have ? *reinterpret_cast<const float4*>(a.B + (size_t)(p / a.bdiv) * a.in + col) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    };
    issue(0);

    f32x4 acc0 = {0.0f, 0.0f, 0.0f, 0.0f}, acc1 = {0.0f, 0.0f, 0.0f, 0.0f};   // two chains: an MFMA waits for its accumulator
    uint8_t* const img = s_img + (size_t)wave * 16 * Gm::PITCH;
    for (int step = 0; step < nsteps; ++step) {
        if (live) {
#pragma unroll
            for (int q = 0; q < Gm::NLD; ++q) {
                const int idx = lane + 64 * q;
                if (idx < 16 * Gm::PIECES) *reinterpret_cast<u32x4*>(img + (idx / Gm::PIECES) * Gm::PITCH + 16 * (idx % Gm::PIECES)) = wpf[q];
            }
        }
#pragma unroll
        for (int q = 0; q < MG_XQ; ++q) {
            const int idx = tid + 64 * MG_WAVES * q;
            *reinterpret_cast<float4*>(s_x + (idx / (MG_STEP / 4)) * MG_XPITCH + 4 * (idx % (MG_STEP / 4))) = xpf[q];
        }
        __syncthreads();   // the step's images are complete
        if (step + 1 < nsteps) issue(step + 1);   // the next step's bytes fly during this step's MFMAs
        if (live) {
            const int col0 = step * MG_STEP;
            const int nsub = min(MG_STEP, a.in - col0) / 32;
            const int shift = (int)((uintptr_t)(my_row + (size_t)step * Gm::SB) & 15u);
            const uint8_t* const st = img + r * Gm::PITCH;
            const float* const xr = s_x + r * MG_XPITCH + 8 * g;   // (r = lane % 16 is also this lane's B / D column)
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                if (FULL || s < nsub) {
                    float w[8];
                    Deq<DT>::run(st, shift, s, g, w);
                    const float4 b0 = *reinterpret_cast<const float4*>(xr + 32 * s), b1 = *reinterpret_cast<const float4*>(xr + 32 * s + 4);
                    const float b[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
                    for (int j = 0; j < 8; ++j) {
                        if (s & 1) acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j], b[j], acc1, 0, 0, 0);
                        else acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(w[j], b[j], acc0, 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();   // every reader is done before the next step's bytes are staged
    }
    if (!live) return;
    // D[i][j]: i = 4 (lane / 16) + reg, j = lane % 16 -- rows row0 + 4 g .. + 3 of the pair in column r
    const int p = s_pair[r];
    if (p < 0) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int row = row0 + 4 * g + e;
        if (row < a.M) {
            float* const o = a.out + (size_t)p * a.M + row;
            float v = acc0[e] + acc1[e];
            if (EPI) { const float gt = *o; v = gt / (1.0f + expf(-gt)) * v; }
            *o = v;
        }
    }
}

// the GEMV form's combine (moe.hip: moe_down_kernel's tail), one thread per output element: the same expression, so the same bits for the same part
__global__ __launch_bounds__(256) void moe_gemm_combine_kernel(float* y, const float* resid, const float* part, const int* ids, const float* w, int T, int hidden,
                                                               int K, int E) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)T * hidden) return;
    const int t = (int)(i / hidden), row = (int)(i % hidden);
    float s = 0.0f;
    for (int k = 0; k < K; ++k) {
        const int p = t * K + k, e = ids[p];
        if (e >= 0 && e < E) s = fmaf(w[p], part[(size_t)p * hidden + row], s);
    }
    y[(size_t)t * hidden + row] = resid[(size_t)t * hidden + row] + s;
}

static bool mg_type_ok(int dt) { return dt == NTK_DT_Q8_0 || dt == NTK_DT_Q4_K || dt == NTK_DT_Q6_K; }
static bool mg_counts_ok(int T, int E, int K) { return T >= 1 && T <= kMgMaxT && E >= 1 && E <= kMgMaxE && K >= 1 && K <= kMgMaxK && K <= E; }

template <int DT, bool EPI>
static void mg_launch_dt(const MoeGemmArgs& a, dim3 grid, hipStream_t st) {
    if (a.in % MG_STEP == 0) hipLaunchKernelGGL((moe_gemm_kernel<DT, true, EPI>), grid, dim3(64 * MG_WAVES), 0, st, a);
    else hipLaunchKernelGGL((moe_gemm_kernel<DT, false, EPI>), grid, dim3(64 * MG_WAVES), 0, st, a);
}

// out[p][0 .. M) (x)= W[e] . B[pairs / bdiv] for every pair of the list; the caller has checked everything
template <bool EPI>
static void mg_launch(int dt, const void* W, const float* B, float* out, const int* offsets, const int* pairs, int M, int in, int bdiv, int n_pairs, int E,
                      hipStream_t st) {
    MoeGemmArgs a{};
    a.W = (const uint8_t*)W; a.B = B; a.out = out; a.offsets = offsets; a.pairs = pairs;
    a.row_bytes = (unsigned)ntk_row_bytes(dt, in);
    a.expert_bytes = (size_t)M * a.row_bytes;
    a.M = M; a.in = in; a.bdiv = bdiv; a.n_pairs = n_pairs; a.E = E;
    const dim3 grid((unsigned)((M + MG_ROWS - 1) / MG_ROWS), (unsigned)moe_tile_bound(n_pairs, E));
    if (dt == NTK_DT_Q8_0) mg_launch_dt<NTK_DT_Q8_0, EPI>(a, grid, st);
    else if (dt == NTK_DT_Q4_K) mg_launch_dt<NTK_DT_Q4_K, EPI>(a, grid, st);
    else mg_launch_dt<NTK_DT_Q6_K, EPI>(a, grid, st);
}

}  // namespace ntk

extern "C" size_t ntk_moe_gemm_scratch_bytes(int T, int E, int K, int inter, int hidden) {
    (void)T; (void)E; (void)K; (void)inter; (void)hidden;
    return 0;   // the gate products wait in act itself
}

extern "C" int ntk_moe_gemm_gate_up(float* act, const float* xn, const void* w_gate, int dt_gate, const void* w_up, int dt_up, const int* offsets,
                                    const int* pairs, void* scratch, size_t scratch_bytes, int T, int hidden, int inter, int E, int K, void* stream) {
    using namespace ntk;
    if (!act || !xn || !w_gate || !w_up || !offsets || !pairs) return NTK_E_NULL;
    if (!mg_type_ok(dt_gate) || !mg_type_ok(dt_up)) return NTK_E_DTYPE;
    if (!mg_counts_ok(T, E, K) || hidden <= 0 || inter <= 0) return NTK_E_SHAPE;
    const size_t rb_g = ntk_row_bytes(dt_gate, hidden), rb_u = ntk_row_bytes(dt_up, hidden);
    if (!rb_g || !rb_u || rb_g > 0x7FFFFFFFu || rb_u > 0x7FFFFFFFu) return NTK_E_SHAPE;   // columns that are not whole blocks
    if (((uintptr_t)act | (uintptr_t)xn) % 16 != 0 || ((uintptr_t)w_gate | (uintptr_t)w_up) % 2 != 0) return NTK_E_ALIGN;
    const size_t need = ntk_moe_gemm_scratch_bytes(T, E, K, inter, hidden);
    if (scratch_bytes < need) return NTK_E_SHAPE;
    if (need && !scratch) return NTK_E_NULL;
    hipStream_t st = resolve_stream(stream);
    mg_launch<false>(dt_gate, w_gate, xn, act, offsets, pairs, inter, hidden, K, T * K, E, st);
    mg_launch<true>(dt_up, w_up, xn, act, offsets, pairs, inter, hidden, K, T * K, E, st);
    return last_launch_status();
}

extern "C" int ntk_moe_gemm_down(float* y, const float* resid, const float* act, const void* w_down, int dt_down, const int* ids, const float* w,
                                 const int* offsets, const int* pairs, float* part, int T, int hidden, int inter, int E, int K, void* stream) {
    using namespace ntk;
    if (!y || !resid || !act || !w_down || !ids || !w || !offsets || !pairs || !part) return NTK_E_NULL;
    if (!mg_type_ok(dt_down)) return NTK_E_DTYPE;
    if (!mg_counts_ok(T, E, K) || hidden <= 0 || inter <= 0) return NTK_E_SHAPE;
    const size_t rb = ntk_row_bytes(dt_down, inter);
    if (!rb || rb > 0x7FFFFFFFu) return NTK_E_SHAPE;
    if ((uintptr_t)act % 16 != 0 || (uintptr_t)w_down % 2 != 0) return NTK_E_ALIGN;
    hipStream_t st = resolve_stream(stream);
    mg_launch<false>(dt_down, w_down, act, part, offsets, pairs, hidden, inter, 1, T * K, E, st);
    const size_t n = (size_t)T * hidden;
    hipLaunchKernelGGL(moe_gemm_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, y, resid, (const float*)part, ids, w, T, hidden, K, E);
    return last_launch_status();
}
