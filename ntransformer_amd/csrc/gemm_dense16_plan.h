// gemm_dense16_plan.h -- layout constants and LAUNCH PLAN of the 16-bit matrix-core prompt GEMM over unquantised F16 / BF16 rows (gemm_dense16.hip): the
// refusals, the tile heights, the grid and its numbering, LDS and workspace bytes -- everything a launch needs that is not a pointer's target.  Plain C++17
// without a HIP header: gemm_dense16.hip and a host test program (tests/gemm_dense16_plan_check.cpp) include it; it reads no environment.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "gemm_f16_plan.h"

namespace ntk {

constexpr int GD_KSTEP = 32;          // columns per matrix instruction (v_mfma_f32_16x16x32_f16 / _bf16): in_features a multiple of this
constexpr int GD_TOK = GB_TOK;        // tokens per workgroup: four token blocks of 16, one chunk of the operand planes
constexpr int GD_WAVES = 4;           // waves per workgroup; a wave owns 16 RT rows x all of the workgroup's tokens
constexpr int GD_MAX_TOKENS = GB_MAX_CHUNKS * GB_TOK;   // one pass (1024)
constexpr int GD_PIECE = GB_PIECE;    // bytes of one (step, plane, token block) operand record: 64 lanes x 8 16-bit words
constexpr int GD_F16_PLANES = GB_PLANES;   // F16 matrices read the FP16 GEMM's own planes (ntk_gemm_prepare_x): two FP16 pieces of x s, 1 / s behind them
constexpr int GD_BF16_PLANES = 3;          // BF16 matrices: three bfloat16 pieces of x, no token scale
constexpr int GD_WANT_WGS = 256;      // the grid the plan aims for: one workgroup per CU

// The token range the callers' dispatch sends here (Dense16Plan.worth; the kernel itself takes any count from 1): below 32 tokens a pass is a stream over the
// weights, narrow matrices (Wo, down: 64 workgroups at 16 rows per wave) leave CUs idle without a K split, and the F32-MFMA form -- one pass over W per 16
// tokens -- is as fast or faster (8B, profiles/dense16_mfma.txt: 16 tokens 15.2 against 10.6 ms; 17 - 24 tokens within the runs' spread; 32 tokens 17.9
// against 19.6 and growing from there).
constexpr int GD_WORTH_TOKENS = 32;
constexpr bool gd_worth(int T) { return T >= GD_WORTH_TOKENS; }

constexpr int gd_planes(int dtype) { return dtype == NTK_DT_BF16 ? GD_BF16_PLANES : GD_F16_PLANES; }
// Workspace.  F16: the FP16 GEMM's layout (gemm_f16_plan.h) -- [chunk][(in / 32 + 1) step records of 8 KB | sums], then [1 / s][s] of the pass.
// BF16: [chunk][in / 32 step records of 12 KB], a record = [plane 0..2][token block 0..3][lane 0..63] x 16 bytes; lane (j, g) of a block holds columns
// 8 g .. 8 g + 7 of the step for token 16 block + j -- the matrix instruction's own operand order, which is also how a row of W lies in memory.
NTK_PLAN_HD constexpr size_t gd_step_bytes(int dtype) { return (size_t)gd_planes(dtype) * 4 * GD_PIECE; }
NTK_PLAN_HD constexpr size_t gd_chunk_bytes(int in, int dtype) {
    return dtype == NTK_DT_BF16 ? (size_t)(in / GD_KSTEP) * gd_step_bytes(dtype) : ws_chunk_bytes(in);
}
NTK_PLAN_HD constexpr size_t gd_inv_offset(int in) { return (size_t)GB_MAX_CHUNKS * ws_chunk_bytes(in); }   // F16: the pass's 1 / s
constexpr size_t gd_workspace_bytes(int in, int dtype) {
    return dtype == NTK_DT_BF16 ? (size_t)GB_MAX_CHUNKS * gd_chunk_bytes(in, dtype) + 256 : gd_inv_offset(in) + GB_SCALE_BYTES + 256;
}
// token blocks a workgroup reads: those the pre-pass writes (split_pad_tokens: whole blocks up to 32 tokens, whole chunks above)
constexpr int gd_ntb(int T) { return T <= 16 ? 1 : (T <= 32 ? 2 : 4); }
constexpr size_t gd_lds_bytes(int dtype, int ntb) { return (size_t)2 * gd_planes(dtype) * ntb * GD_PIECE; }   // two step records: one read, one being filled

struct Dense16SegPlan { int tile0, tiles; };   // first workgroup row tile of this matrix in the launch's numbering; its row tiles
struct Dense16Plan {
    int status;            // NTK_OK or the refusal: nothing else is set
    int dtype, planes;
    bool worth;            // this token count is routed here rather than to the F32-MFMA form (gd_worth)
    int rt, ntb;           // 16 rt rows per wave (64 rt per workgroup); token blocks per workgroup
    int steps;             // in / 32
    int tiles, chunks;     // row tiles of all matrices; 64-token chunks
    unsigned grid_x, block;
    size_t lds;
    size_t step_bytes, chunk_bytes, ws_bytes;   // the workspace the launch addresses: chunks x chunk_bytes (+ F16: the scales at gd_inv_offset)
    Dense16SegPlan seg[GB_MAX_SEG];
};

// where workgroup b of the grid works: the eight XCDs take workgroups round robin, so the row tile is numbered in the low three bits and every chunk of a
// row tile lands on ONE XCD, whose L2 then holds that tile's weights once.  false: b is padding (tiles rounded up to eight)
NTK_PLAN_HD inline bool gd_map(unsigned b, int tiles, int chunks, int& tile, int& chunk) {
    const unsigned slot = b >> 3;
    tile = (int)(slot / (unsigned)chunks) * 8 + (int)(b & 7u);
    chunk = (int)(slot % (unsigned)chunks);
    return tile < tiles;
}

// 1 <= T <= 1024 tokens; nseg matrices [rows_i][in] of ONE 16-bit dtype sharing X; ptrs: every pointer of the call (W_i, Y_i, X, resid, workspace).
// Refused, in this order: NTK_E_DTYPE (a dtype that is not F16 / BF16, or two of them in one call), NTK_E_SHAPE (segments outside 1 .. 3, rows that are
// not whole tiles of 16, in_features that is not whole steps of 32, T outside one pass), NTK_E_ALIGN (a pointer off the 16-byte grid).
inline Dense16Plan gemm_dense16_plan(const int* rows, const int* dtypes, int nseg, int T, int in, const uintptr_t* ptrs = nullptr, int nptr = 0) {
    Dense16Plan p{};
    p.status = NTK_E_SHAPE;
    if (nseg < 1 || nseg > GB_MAX_SEG) return p;
    for (int i = 0; i < nseg; ++i)
        if ((dtypes[i] != NTK_DT_F16 && dtypes[i] != NTK_DT_BF16) || dtypes[i] != dtypes[0]) { p.status = NTK_E_DTYPE; return p; }
    if (in <= 0 || in % GD_KSTEP != 0 || T < 1 || T > GD_MAX_TOKENS) return p;
    for (int i = 0; i < nseg; ++i)
        if (rows[i] <= 0 || rows[i] % 16 != 0) return p;
    for (int i = 0; i < nptr; ++i)
        if (ptrs[i] & 15) { p.status = NTK_E_ALIGN; return p; }
    p.status = NTK_OK;
    p.dtype = dtypes[0]; p.planes = gd_planes(p.dtype);
    p.steps = in / GD_KSTEP;
    p.worth = gd_worth(T);
    p.ntb = gd_ntb(T);
    p.chunks = (T + GD_TOK - 1) / GD_TOK;
    // Rows per wave: the tallest tile (64 rows: a weight fragment then feeds planes x 4 token blocks of matrix instructions, and a step record read from
    // LDS four row tiles) that still gives every CU a workgroup; narrower launches take shorter tiles down to 16 rows per wave.
    auto tiles_at = [&](int rt) { int n = 0; for (int i = 0; i < nseg; ++i) n += (rows[i] + 64 * rt - 1) / (64 * rt); return n; };
    int rt = 4;
    while (rt > 1 && (long)tiles_at(rt) * p.chunks < GD_WANT_WGS) rt >>= 1;
    p.rt = rt;
    int tiles = 0;
    for (int i = 0; i < nseg; ++i) { p.seg[i].tile0 = tiles; p.seg[i].tiles = (rows[i] + 64 * rt - 1) / (64 * rt); tiles += p.seg[i].tiles; }
    p.tiles = tiles;
    p.grid_x = (unsigned)((tiles + 7) / 8 * 8 * p.chunks); p.block = 64 * GD_WAVES;
    p.lds = gd_lds_bytes(p.dtype, p.ntb);
    p.step_bytes = gd_step_bytes(p.dtype); p.chunk_bytes = gd_chunk_bytes(in, p.dtype); p.ws_bytes = gd_workspace_bytes(in, p.dtype);
    return p;
}

}  // namespace ntk
