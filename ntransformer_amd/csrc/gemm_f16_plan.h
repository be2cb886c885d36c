// gemm_f16_plan.h -- the prompt GEMM's layout constants, per-format numbers and LAUNCH PLAN (gemm_f16.hip): which of the three kernel forms a call takes,
// its tile height, K slices, grid, LDS bytes and the segments' tile numbering -- everything a launch needs that is not a pointer.  Plain C++17 without a
// HIP header: gemm_f16.hip and a host test program (tests/gemm_plan_check.cpp, tests/golden/gemm_f16_plans.txt) include it; it reads no environment.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <algorithm>
#include "../../include/ntk.h"

#ifdef __HIPCC__
#define NTK_PLAN_HD __host__ __device__
#else
#define NTK_PLAN_HD
#endif

namespace ntk {

constexpr int GB_TOK = 64;           // tokens per pass
// K splits x 64-token chunks of one launch never exceed this (size of the partial-sum area): 32 for matrices of up to 8192 rows (the narrow
// ones are the ones that need splits at many chunks), 16 above
constexpr int gb_split_rows(int out_total) { return out_total <= 8192 ? 32 : 16; }
constexpr int GB_MAX_CHUNKS = 16;   // 64-token chunks per launch (32 measured no better: 15.1k vs 16.0k tok/s at 2048 tokens)
constexpr int GB_PIECE = 1024;       // bytes of one (step, plane, token block) operand record
constexpr int GB_PLANES = 2;         // FP16 pieces of an activation
constexpr int GB_STEP_BYTES = GB_PLANES * 4 * GB_PIECE;   // 8 KB of activation operands per step
constexpr int GB_WG_PER_CU = 2, GB_LDS_WG = 80 * 1024, GB_NRING_Q8 = 2;   // two workgroups (8 waves) per CU; Q8_0: units in flight per wave
constexpr int GB_AUX_BYTES = GB_TOK * 4;                  // per step: one eighth of its unit's record of sums (K-quant minimum term)
constexpr int GB_MIN_UNIT_BYTES = 8 * GB_AUX_BYTES;       // per unit of 8 steps and 64-token chunk: 2 pieces x 4 token blocks x 2 x 16 tokens x 4 steps x FP16
constexpr size_t GB_SCALE_BYTES = 2 * GB_MAX_CHUNKS * GB_TOK * sizeof(float);   // the launch's 1 / s and s
constexpr int GB_MAX_SEG = 3;   // matrices sharing X in one launch (Q | K | V, gate | up)
constexpr int GB_UPT = 2;     // units per loop trip (Q6_K: the parity of a unit, which decides its alignment, is then a compile-time constant)
constexpr int GB_RP = 32;   // DT + GB_RP = the same format read from the repack (internal to gemm_f16.hip)
#ifdef NTK_GEMM_TRACE       // (make trace: the step timeline's stamps sit in LDS behind the waves' images)
constexpr int GBT_STEPS = 96, GBT_EV = 3;
constexpr int GB_TRACE_LDS = 4 * GBT_STEPS * GBT_EV * 8;
#else
constexpr int GB_TRACE_LDS = 0;
#endif

// Layout of the workspace: [chunk][(in / 32 + 1) step records of 8 KB | sums of the units], then [1 / s][s] of the pass.
// one chunk's planes + sums (+ the record of zeros), rounded to 256 B
// (the sums: whole units of 8 steps covering steps 0 .. in/32 + 7 -- the pre-pass writes a full unit of zeros behind the last step)
NTK_PLAN_HD constexpr size_t ws_chunk_bytes(int in) {
    return ((size_t)(in / 32 + 1) * GB_STEP_BYTES + (size_t)((in / 32 + 15) / 8) * GB_MIN_UNIT_BYTES + 255) / 256 * 256;
}
// tokens of the launch rounded up to the token blocks the matrix instructions read (16 per block; the 64-token form reads whole chunks)
constexpr int split_pad_tokens(int T) { return T <= 32 ? (T + 15) / 16 * 16 : (T + GB_TOK - 1) / GB_TOK * GB_TOK; }

// ---- per-format numbers (each DeqI<DT> of gemm_f16.hip inherits its own) --------------------------------------------------
// BW, BB: columns and bytes of a block; SPU: 32-column steps per unit (whole blocks: Q8_0 4 blocks, Q4_0 8, the K-quants one super-block); STRIDE:
// bytes between the row images of a wave's LDS image; ROW_ALIGN: the row pitch at which the decoders' LDS dword reads are aligned; SPLIT16: scales per
// 16 columns; HAS_MIN: a K-quant minimum term; PF: the plane prefetch of the chunk form; RP: read from the decode repack, whose items are ITEM =
// 2 S1 + S2 bytes per tile of 16 rows and super-block (S1: a step's nibble plane and its high bits, S2: the rows' records).
template <int DT> struct GemmFmt;
template <> struct GemmFmt<NTK_DT_Q8_0> {
    static constexpr int BW = 32, BB = 34, SPU = 4, STRIDE = 176, ROW_ALIGN = 4;     // row pitch: in_features a multiple of 64
    static constexpr bool SPLIT16 = false, HAS_MIN = false, PF = true;
    static constexpr bool RP = false; static constexpr int ITEM = 0, S1 = 0, S2 = 0;
};
template <> struct GemmFmt<NTK_DT_Q4_0> {
    static constexpr int BW = 32, BB = 18, SPU = 8, STRIDE = 176, ROW_ALIGN = 4;     // row pitch: in_features a multiple of 64
    static constexpr bool SPLIT16 = false, HAS_MIN = false, PF = true;
    static constexpr bool RP = false; static constexpr int ITEM = 0, S1 = 0, S2 = 0;
};
template <> struct GemmFmt<NTK_DT_Q4_K> {
    static constexpr int BW = 256, BB = 144, SPU = 8, STRIDE = 144, ROW_ALIGN = 16;  // rows are 16-byte aligned: no shift
    static constexpr bool SPLIT16 = false, HAS_MIN = true, PF = true;
    static constexpr bool RP = false; static constexpr int ITEM = 0, S1 = 0, S2 = 0;
};
template <> struct GemmFmt<NTK_DT_Q5_K> {
    static constexpr int BW = 256, BB = 176, SPU = 8, STRIDE = 176, ROW_ALIGN = 16;  // rows are 16-byte aligned: no shift
    static constexpr bool SPLIT16 = false, HAS_MIN = true, PF = true;
    static constexpr bool RP = false; static constexpr int ITEM = 0, S1 = 0, S2 = 0;
};
template <> struct GemmFmt<NTK_DT_Q6_K> {
    static constexpr int BW = 256, BB = 210, SPU = 8, STRIDE = 240, ROW_ALIGN = 4;   // row pitch: in_features a multiple of 512
    static constexpr bool SPLIT16 = true, HAS_MIN = false, PF = false;
    static constexpr bool RP = false; static constexpr int ITEM = 0, S1 = 0, S2 = 0;
};
template <> struct GemmFmt<NTK_DT_Q4_K + GB_RP> {
    static constexpr bool RP = true;
    static constexpr int S1 = 1024, S2 = 320, ITEM = 2 * S1 + S2;
    static constexpr int BW = 256, BB = 144, SPU = 8, STRIDE = ITEM / 16, ROW_ALIGN = 16;
    static constexpr bool SPLIT16 = false, HAS_MIN = true, PF = true;
};
template <> struct GemmFmt<NTK_DT_Q5_K + GB_RP> {
    static constexpr bool RP = true;
    static constexpr int S1 = 1280, S2 = 320, ITEM = 2 * S1 + S2;
    static constexpr int BW = 256, BB = 176, SPU = 8, STRIDE = ITEM / 16, ROW_ALIGN = 16;
    static constexpr bool SPLIT16 = false, HAS_MIN = true, PF = true;
};
template <> struct GemmFmt<NTK_DT_Q6_K + GB_RP> {
    static constexpr bool RP = true;
    static constexpr int S1 = 1536, S2 = 288, ITEM = 2 * S1 + S2;
    static constexpr int BW = 256, BB = 210, SPU = 8, STRIDE = ITEM / 16, ROW_ALIGN = 16;
    static constexpr bool SPLIT16 = true, HAS_MIN = false, PF = false;
};

// ---- LDS of the three kernel forms ----------------------------------------------------------------------------------------------------
// Chunk form.  LDS of a workgroup: a ring of NS activation step records (8 KB each, filled by LDS-DMA NS - 1 steps ahead), the ring of the steps'
// per-token sums, the 4 waves' weight images.  NS = as many slots as leave room for two workgroups per CU (160 KB): a record that
// misses the XCD's L2 takes ~2 us to arrive, and the records in flight are what hides it (a step consumes one in 0.3-0.4 us)
// CW = 64-token chunks per workgroup (1 or 2: a slot then holds the records of both)
template <int DT, int CW> constexpr int gb_aux_lds() { return GemmFmt<DT>::HAS_MIN ? CW * 2 * GB_MIN_UNIT_BYTES : 0; }   // two units of sums per chunk
template <int DT, int RT, int CW> constexpr int gb_slots() {
    const int n = (GB_LDS_WG - 4 * 16 * RT * GemmFmt<DT>::STRIDE - GB_TRACE_LDS - gb_aux_lds<DT, CW>()) / (CW * GB_STEP_BYTES);
    return n > 8 ? 8 : (n < 3 ? 3 : n);
}
template <int DT, int RT, int CW> constexpr int gb_lds_bytes() {
    return gb_slots<DT, RT, CW>() * CW * GB_STEP_BYTES + gb_aux_lds<DT, CW>() + 4 * 16 * RT * GemmFmt<DT>::STRIDE + GB_TRACE_LDS;
}
// Small form: nw waves x (the wave's weight image + its partial sums)
template <int DT> constexpr int gs_lds_bytes(int rt, int ntb, int nw) { return nw * (16 * rt * GemmFmt<DT>::STRIDE + ntb * rt * 1024); }
template <int DT, int RT, int NTB> constexpr int gs_lds_bytes(int nw) { return gs_lds_bytes<DT>(RT, NTB, nw); }
// K-slice form: units of weights in flight per wave (registers)
constexpr int GK_DEPTH4 = 4;   // units of 4 steps (Q8_0: 2176 B per 16 rows) in flight per wave
constexpr int GK_DEPTH8 = 2;   // units of 8 steps
template <int SPU> constexpr int gk_depth() { return SPU <= 4 ? GK_DEPTH4 : GK_DEPTH8; }
// waves per workgroup: 8.  (16 -- four per SIMD at <= 128 registers, for the 16 rows x 16 tokens form -- measured SLOWER, same box, alternated twice: 8B Q8_0
// 16 tokens 4.74 -> 5.60 ms, Q4_K_M 4.26 -> 4.66: twice the slices at half the length.  GK_WAVES_RT1 = 16 rebuilds it.  profiles/r06_prompt_kslice.txt)
constexpr int GK_WAVES_RT1 = 8;
template <int DT> constexpr int gk_waves(int rt, int ntb) { return rt == 1 && ntb == 1 && !(GemmFmt<DT>::SPLIT16 && !GemmFmt<DT>::RP) ? GK_WAVES_RT1 : 8; }
template <int DT, int RT, int NTB> constexpr int gk_waves() { return gk_waves<DT>(RT, NTB); }
template <int DT> constexpr int gk_lds_bytes(int rt, int ntb, int nw, int slice_steps) {
    return slice_steps * GB_PLANES * ntb * GB_PIECE + nw * (16 * rt * GemmFmt<DT>::STRIDE);
}
template <int DT, int RT, int NTB> constexpr int gk_lds_bytes(int nw, int slice_steps) { return gk_lds_bytes<DT>(RT, NTB, nw, slice_steps); }
// steps of planes that fit beside the waves' images in the CU's 160 KB (whole units).  The images are counted at 256 bytes per row whatever the format
// (176 .. 240 in fact): the raw GGUF form of a matrix and its decode repack then get the SAME slices -- and with them the same sums in the same order.
template <int DT> constexpr int gk_max_steps(int rt, int ntb) {
    static_assert(GemmFmt<DT>::STRIDE <= 256, "a row image is counted at 256 bytes");
    return (160 * 1024 - gk_waves<DT>(rt, ntb) * (16 * rt * 256)) / (GB_PLANES * ntb * GB_PIECE) / GemmFmt<DT>::SPU * GemmFmt<DT>::SPU;
}
template <int DT, int RT, int NTB> constexpr int gk_max_steps() { return gk_max_steps<DT>(RT, NTB); }
// two 64-token chunks per workgroup (chunk form): not the formats that scale per 16 columns; Q5_K: 15 registers over the budget in that form
template <int DT> constexpr bool gb_cw2_ok() { return !GemmFmt<DT>::SPLIT16 && DT != NTK_DT_Q5_K && DT != NTK_DT_Q5_K + GB_RP; }

// ---- the plan ---------------------------------------------------------------------------------------------------------------------------
// The tuning switches of tuning builds (make tune; the environment variable NTK_GEMM_<NAME> of each is read where gemm_f16.hip builds this struct);
// the values below are the product's.
struct GemmTune {
    int kslice = -1;                                   // KSLICE: 0 = never the K-slice form, n = up to n tokens
    int kslice_c0 = 32, kslice_c1 = 8;                 // KSLICE_C0, KSLICE_C1: the cost model's fixed parts, in steps
    int kslice_rt = 0, kslice_n = 0, kslice_jobs = 64; // KSLICE_RT, KSLICE_N: forced; KSLICE_JOBS = 1: one row group per workgroup
    int small = -1, small_rt = 0, small_nw = 0;        // SMALL: 0 = never the small form, n = up to n tokens; SMALL_RT, SMALL_NW: forced
    int map = 1, rt = 0, wgs = 0, no_pf = 0, cw = 0;   // MAP, RT, WGS, NO_PF (the A/B switch of the plane prefetch), CW: the chunk form
};
enum GemmForm { GEMM_FORM_KSLICE = 0, GEMM_FORM_SMALL = 1, GEMM_FORM_CHUNK = 2 };
struct GemmSegPlan {
    int tile0, tiles16;     // first row tile of this matrix in the launch's tile numbering; its tiles of 16 rows
    unsigned w_last;        // out * row_bytes - 16: the last 16-byte piece of the matrix (requests past the end re-read it)
    unsigned p2_off;        // repacked tensors: byte offset of the row records behind the nibble planes (csrc/gemv_rp.hip: P1 of every item, then P2)
    size_t part_off;        // floats from the start of the partial-sum area to this matrix's [nsplit][T][out]
};
struct GemmPlan {
    int status;             // NTK_OK, or NTK_E_SHAPE: nothing else is set
    int form;               // GemmForm
    int rt, ntb, cw;        // 16 rt rows per wave; token blocks of the short forms (0: chunk form); chunks per workgroup (0: short forms)
    bool al, pf;            // rows on dword boundaries; the plane prefetch (chunk form)
    int nsplit, per_split;  // K slices (grid y); units per slice (K-slice form) / steps per split (chunk form)
    int jobs, waves;        // row groups per workgroup (K-slice form); waves per workgroup
    unsigned grid_x, grid_y, block;
    size_t lds;             // dynamic LDS bytes
    int tiles, chunks;      // row tiles of all matrices; chunks (chunk form: of 64 cw tokens) along the grid
    unsigned row_bytes;
    GemmSegPlan seg[GB_MAX_SEG];
};

// the matrices' tiles of `tile_rows` rows, numbered through; returns their count
template <int DT> inline int gemm_plan_segs(GemmPlan& p, const int* rows, int nseg, int in, int tile_rows) {
    int tiles = 0;
    for (int i = 0; i < nseg; ++i) {
        p.seg[i].w_last = (unsigned)((size_t)rows[i] * p.row_bytes - 16);
        p.seg[i].tiles16 = rows[i] / 16;
        p.seg[i].p2_off = (unsigned)((size_t)p.seg[i].tiles16 * (size_t)(in / 256) * (size_t)(2 * GemmFmt<DT>::S1));
        p.seg[i].tile0 = tiles;
        tiles += (rows[i] + tile_rows - 1) / tile_rows;
    }
    return tiles;
}
// partial-sum areas, one after the other: nsplit x T x out_i floats each
inline void gemm_plan_parts(GemmPlan& p, const int* rows, int nseg, int T) {
    size_t off = 0;
    for (int i = 0; i < nseg; ++i) {
        p.seg[i].part_off = off;
        off += (size_t)p.nsplit * T * rows[i];
    }
}

// T <= GB_MAX_CHUNKS * 64 = 1024 tokens in one launch; nseg matrices [rows_i][in] of format DT sharing X.
// (full_form: the form, K split and chunk pairing of a full pass -- GB_MAX_CHUNKS chunks -- whatever T is, never the short-prompt forms: a token's
// sums then run in the same order however the caller cuts its tokens into calls -- ntk_gemm_desc.full_form)
template <int DT>
inline GemmPlan gemm_f16_plan(const int* rows, int nseg, int T, int in, bool full_form, const GemmTune& tune) {
    using D = GemmFmt<DT>;
    GemmPlan p{};
    p.status = NTK_E_SHAPE;
    // whole units only (Q8_0: in a multiple of 128, Q4_0 and the K-quants: of 256): a partial last unit would decode the next row's bytes as
    // scales -- any bit pattern, NaNs included -- against the zero activations of the padding steps
    if (nseg < 1 || nseg > GB_MAX_SEG || in % (32 * D::SPU) != 0) return p;
    const size_t row_bytes = (size_t)in / D::BW * D::BB;
    long out_total = 0;
    for (int i = 0; i < nseg; ++i) {
        if (rows[i] <= 0 || rows[i] % 16 != 0 || (size_t)rows[i] * row_bytes > 0xFFFFFF00ull) return p;   // 32-bit piece offsets
        if (D::RP && (size_t)(rows[i] / 16) * (size_t)(in / 256) * (size_t)D::ITEM > 0xFFFFFFF0ull) return p;
        out_total += rows[i];
    }
    p.status = NTK_OK;
    p.row_bytes = (unsigned)row_bytes;
    p.jobs = 1; p.chunks = 1; p.grid_y = 1;
    // AL: every row starts on a dword boundary, so that the decoders' LDS dword reads are aligned (Q8_0 / Q4_0: in a multiple of 64, Q6_K: of
    // 512 -- every projection of the target models; other row pitches take the same kernel with 2-byte aligned reads, slower)
    p.al = D::RP || row_bytes % D::ROW_ALIGN == 0;
    const int ntb = T <= 16 ? 1 : 2;   // token blocks of the short forms

    // ---- short prompts (<= 32 tokens), second form: K-slice-stationary (gemm_quant_f16_kslice_kernel) ----
    // Plan: RT (16 or 32 rows per wave) and the number of K slices, by a two-term model of the launch -- rounds of workgroups over the 256 CUs x (steps of
    // a slice x RT + a fixed part worth `c0` steps: the copy of the planes, the first weights' round trip, the partial sums) -- over the slice counts that
    // keep the planes within LDS (gk_max_steps: 64 / NTB steps beside 16-row images, 48 / NTB beside 32-row ones) and the partial sums within their area.
    // (Four token blocks -- 33 .. 64 tokens -- were built and measured as well: 8B Q8_0 64 tokens 6.38 -> 8.74 ms, Q4_K_M 6.75 -> 9.57: 16-step slices, 8 - 28 of
    // them per matrix, and up to 58 MB of partial sums per launch; the 64-token chunk form keeps those.  profiles/r06_prompt_kslice.txt)
    const int kslice_max = tune.kslice >= 0 ? tune.kslice : 32;
    if (!full_form && T <= kslice_max && T <= 32) {
        const int units = in / (32 * D::SPU);
        const int c0 = tune.kslice_c0, c1 = tune.kslice_c1, max_jobs = tune.kslice_jobs;
        int best_n = 0, best_rt = 0, best_ups = 0, best_jobs = 1;
        double best_cost = 1e30;
        for (int krt = 1; krt <= 2; ++krt) {
            if (tune.kslice_rt && krt != tune.kslice_rt) continue;
            // over the register budget (the build's ISA shows spills): 32 rows x 32 tokens of the K-quant decoders; the raw Q6_K decoder beyond 16 x 16
            // (Q6_K: the same rule for the raw tensor and its repack -- they must take the same slices to give the same bits)
            if ((krt == 2 && ntb >= 2 && (D::SPLIT16 || D::HAS_MIN)) || (D::SPLIT16 && (krt == 2 || ntb >= 2))) continue;
            int kt = 0;
            for (int i = 0; i < nseg; ++i) kt += (rows[i] + 16 * krt - 1) / (16 * krt);
            const int max_steps = gk_max_steps<DT>(krt, ntb), knw = gk_waves<DT>(krt, ntb);
            const int wgx = (kt + knw - 1) / knw, max_units = max_steps / D::SPU;
            if (max_units < 1) continue;
            const int n_min = (units + max_units - 1) / max_units, n_cap = std::min(units, gb_split_rows((int)out_total));
            for (int n = n_min; n <= n_cap; ++n) {
                const int ups = units / n;
                if (units % n != 0 || ups % gk_depth<D::SPU>() != 0 || (tune.kslice_n && n != tune.kslice_n)) continue;   // (equal slices of whole groups of units)
                // rounds over the 256 CUs, folded into the workgroups (the planes are copied once): the fewest row groups per workgroup with which
                // the whole grid -- ceil(wgx / jobs) x n -- is ONE round
                int jobs = 1;
                while (jobs < max_jobs && (long)((wgx + jobs - 1) / jobs) * n > 256) ++jobs;
                const double cost = (double)jobs * (double)(ups * D::SPU * krt) + c0 + (jobs - 1) * c1;
                if (cost < best_cost) { best_cost = cost; best_n = n; best_rt = krt; best_ups = ups; best_jobs = jobs; }
            }
        }
        if (best_n > 0) {
            p.form = GEMM_FORM_KSLICE; p.rt = best_rt; p.ntb = ntb;
            p.nsplit = best_n; p.per_split = best_ups; p.jobs = best_jobs;
            p.tiles = gemm_plan_segs<DT>(p, rows, nseg, in, 16 * best_rt);
            gemm_plan_parts(p, rows, nseg, T);
            p.waves = gk_waves<DT>(best_rt, ntb);
            const int kwgx = (p.tiles + p.waves - 1) / p.waves;
            p.grid_x = (unsigned)((kwgx + best_jobs - 1) / best_jobs); p.grid_y = (unsigned)best_n; p.block = (unsigned)(64 * p.waves);
            p.lds = gk_lds_bytes<DT>(best_rt, ntb, p.waves, best_ups * D::SPU);
            return p;
        }
    }
    // ---- short prompts (<= 32 tokens): the weight-streaming form (gemm_quant_f16_small_kernel) ----
    // Measured (profiles/r06_prompt_small_tokens.txt, same box): <= 16 tokens it wins for every format (8B Q8_0 16 tokens 5.99 -> 5.53 ms per pass, the F32-MFMA
    // form of rounds 1-5: 7.18; 8B Q4_K_M 6.39 -> 5.22; 70B Q4_K_M 37.3 -> 28.4); with two token blocks (17 .. 32 tokens) only for the K-quant decoders
    // (8B Q4_K_M 32 tokens 6.45 -> 5.73 ms; Q8_0 6.09 -> 6.23: the 64-token form keeps those).  It streams at 1.4-2.4 TB/s, not at the decode GEMV's 4-6: a
    // wave's steps each wait for their activation planes' L2 round trip (one step ahead is 100 cycles of work against ~600), and a ring of four units of
    // weights in flight per wave changed nothing -- the next step up needs the planes resident in LDS, i.e. the large kernel's structure.
    const int small_max = tune.small >= 0 ? tune.small : ((D::HAS_MIN || D::SPLIT16) ? 32 : 16);
    if (!full_form && T <= small_max && T <= 32) {
        int srt = tune.small_rt ? tune.small_rt : (out_total >= 16384 ? 2 : 1);
        if (D::SPLIT16 && T > 16) srt = 1;   // (32 rows x 32 tokens of the format that scales per 16 columns: over the register budget)
        const int units = in / 32 / D::SPU;
        const int snw = std::min(8, tune.small_nw ? std::min(tune.small_nw, std::max(1, units)) : std::min(8, std::max(1, units)));   // (__launch_bounds__(512))
        p.form = GEMM_FORM_SMALL; p.rt = srt; p.ntb = ntb;
        p.nsplit = 1;   // (K is split inside the launch, over the waves)
        p.tiles = gemm_plan_segs<DT>(p, rows, nseg, in, 16 * srt);
        p.waves = snw;
        p.grid_x = (unsigned)p.tiles; p.block = (unsigned)(64 * snw);
        p.lds = gs_lds_bytes<DT>(srt == 2 ? 2 : 1, ntb, snw);
        return p;
    }
    // ---- the chunk form (gemm_quant_f16_kernel) ----
    // Rows per wave (RT x 16): a workgroup streams ALL B operands of its K range from L2 whatever its height, so taller tiles
    // cut that traffic and the LDS reads per MFMA; K is then split (in whole trips) while fewer than one workgroup per CU exists.
    // K is split (in whole trips) until every CU has two workgroups -- from 4 chunks (193 tokens) on; below that one per CU: the partial
    // sums of many splits cost more than the idle half buys (same box, 8B Q8_0: 256 tokens 16 370 -> 17 000 tok/s, 512 19 830 -> 20 950;
    // 64 tokens 8 090 -> 7 570 with the same rule, which is why it stops there)
    constexpr int TRIP = GB_UPT * D::SPU;   // steps per loop trip: K ranges are whole trips
    p.chunks = (T + GB_TOK - 1) / GB_TOK;
    const int plan_chunks = full_form ? GB_MAX_CHUNKS : p.chunks;   // the chunk count the plan below is made for
    const int want_wgs = tune.wgs ? tune.wgs : (plan_chunks >= 4 ? 512 : 256);
    int rt = out_total >= 2048 ? 2 : 1;
    if (tune.rt == 1 || tune.rt == 2) rt = tune.rt;
    p.tiles = gemm_plan_segs<DT>(p, rows, nseg, in, 64 * rt);
    const int trips = (in / 32 + TRIP - 1) / TRIP;
    // K splits of a plan with `groups` workgroup columns: doubled while the grid is short of `want_wgs`, whole trips, and
    // splits x 64-token chunks within the partial-sum area (gb_split_rows)
    const int chunks64 = plan_chunks, max_rows = gb_split_rows((int)out_total);
    auto splits_for = [&](int groups) {
        int n = 1;
        while (n * 2 * chunks64 <= max_rows && (long)p.tiles * groups * n < want_wgs && trips / (n * 2) >= 1) n *= 2;
        return n;
    };
    // two chunks (128 tokens) per workgroup when that still gives every CU two workgroups -- directly, or (narrow matrices: the 8B down /
    // o / Q|K|V projections at 1024 tokens) with K split in two
    int nsplit = splits_for(chunks64);
    bool cw2 = false;
    if (gb_cw2_ok<DT>() && p.al && rt == 2 && chunks64 >= 2 && tune.cw != 1) {
        const int pairs = (chunks64 + 1) / 2, n2 = splits_for(pairs);
        if ((n2 <= 2 && (long)p.tiles * pairs * n2 >= 512) || tune.cw == 2) { cw2 = true; nsplit = n2; p.chunks = (p.chunks + 1) / 2; }
    }
    const int tps = (trips + nsplit - 1) / nsplit;   // trips per split
    nsplit = (trips + tps - 1) / tps;                // no empty split
    p.form = GEMM_FORM_CHUNK; p.rt = rt; p.ntb = 0; p.cw = cw2 ? 2 : 1;
    p.pf = !cw2 && D::PF && !(p.al && tune.no_pf);
    p.nsplit = nsplit; p.per_split = tps * TRIP;
    gemm_plan_parts(p, rows, nseg, T);
    p.waves = 4;
    p.grid_x = (unsigned)((p.tiles + 7) / 8 * 8 * p.chunks); p.grid_y = (unsigned)nsplit; p.block = 256;
    p.lds = cw2 ? gb_lds_bytes<DT, 2, 2>() : (rt == 2 ? gb_lds_bytes<DT, 2, 1>() : gb_lds_bytes<DT, 1, 1>());
    return p;
}

}  // namespace ntk
