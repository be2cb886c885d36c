// gemv.hip -- dequant-fused GEMV for batch-1 decode on gfx950 (CDNA4, wave64).
//
// Replaces: launch_gemv / launch_gemv_add and the seven gemv_*_kernel of the reference
// (reference src/cuda/gemm.cu:32-671, 748-871).  Same inputs (RAW GGUF blocks, row-major [out][in], F32 x)
// and the same per-block arithmetic (integer quant x F32 activation, F32 accumulate, FP16 scale applied per
// block / sub-block); the decomposition is new:
//
//   * A lane owns 64 consecutive COLUMNS of a <=4096-column slice for the whole launch, so its 64
//     activations (optionally RMS-normalised on the fly) live in VGPRs; the reference re-reads x from
//     shared memory for every weight (4 B of LDS traffic per weight).
//   * A wave streams the slice of each row it owns as a BYTE stream: coalesced 16 B/lane non-temporal
//     loads (1 KiB per wave instruction), software-prefetched one row ahead into VGPRs.  GGUF blocks are
//     34/18/144/176/210 bytes and only 2-byte aligned, so the stream is bounced through a wave-private LDS
//     image (ds_write_b128, no barrier: a wave's DS ops execute in order) and each lane pulls the bytes of
//     ITS columns back with aligned dword reads + v_alignbyte.  LDS carries ~2 B per weight byte instead
//     of 4 B per weight; the reference's "lane b reads block b" pattern would be a 34-byte-stride gather.
//   * Rows longer than 4096 columns are split across the waves of one workgroup (slice s = wave % ns);
//     partial sums meet in LDS once per batch of 4 rows (one barrier, fixed summation order).
//   * Fusions the engine uses (ntk_gemv_fused): RMSNorm prologue, Q|K|V or gate|up row segments sharing
//     one x, residual-add epilogue, SiLU(gate)*up epilogue.
//   * A decode launch lasts 6-22 us, so its first 3 us are designed like the loop: the activations are requested first thing
//     (only the register quads the row needs), have landed before a wave requests its first weight row (a CU returns loads in
//     request order), reach the lanes through a padded LDS image beside the staging areas, and the bookkeeping runs under
//     their latency.  make trace + tools/gemv_trace.py print the timeline of a launch inside a hipGraph chain.
//
// HBM-bound: algorithmic bytes per launch = rows * row_bytes (+ in*4 for x per workgroup from L2).
#include "gemv_core.hip.h"
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstddef>
#include <mutex>
#include <cstdio>
#include <cstdlib>

namespace ntk {

// ------------------------------------------------------------------------------------------------
// The kernel.  blockDim.x = 64 * ns * rw.  Dynamic LDS:
//   [0, A)   the activation image of the prologue and nwaves * STAGE wave-private images of row bytes (side by side for rows of
//            one column slice, the staging areas over the image -- behind a barrier -- for wider rows)
//   [A, ..)  partial sums [2][rw][ns][RB] + 16 floats reduction scratch
// ------------------------------------------------------------------------------------------------
// LM: the lane-major Q8_0 repack (gemv_core.hip.h: q8l_layout) -- the same kernel with the row transport replaced: a lane loads its own 64 quants (four
// coalesced 16-byte requests) and its two scales (one dword) straight into registers; no staging areas, no ds_write / read-back / realign.
//
// NSF: whether a row is one slice, as a compile-time choice for the lane-major kernels -- each instantiation carries only its own row loop and
// epilogue (one kernel for both held 128 VGPRs with 3-4 of them spilled to scratch: a private segment on the headline's hottest launches)
//   NS_ANY    decided at run time from p.ns (the kernels over GGUF blocks)
//   NS_ONE    rows of one slice: a wave owns whole rows
//   NS_SPLIT  rows of several slices, one wave per slice, partial sums combined through LDS
enum { NS_ANY = 0, NS_ONE = 1, NS_SPLIT = 2 };

// The static decode activations (ntk_decode_arena_*, ntk_engine.h): the single-token vectors the decode GEMVs read as x, at an address the
// kernel knows at link time.  A workgroup's kernel arguments are cold every token (0.5-0.8 us), and x's address is one of them: with x in a
// slot, the x requests go out in the kernel's first instructions and land while the arguments are still on their way -- two round trips side
// by side instead of one after the other.  XS names the slot of an "early-x" form and fixes its column count (the 8B shapes):
//   XS_HIDDEN    the hidden state behind a fused RMSNorm, 4096 columns (Q|K|V, gate|up, LM head: every reader of it)
//   XS_ATTN      the attention output, 4096 columns (Wo)
//   XS_GATE      SiLU(gate) x up, 14336 columns (down)
// The host (q8l_gemv_fused) picks a form only when the call's x IS that slot and `in` is that count; 512 threads per workgroup.
enum { XS_NONE = 0, XS_HIDDEN = NTK_ARENA_HIDDEN, XS_ATTN = NTK_ARENA_ATTN_OUT, XS_GATE = NTK_ARENA_GATE };
struct DecodeArena {
    float hidden[NTK_ARENA_HIDDEN_FLOATS];
    float attn_out[NTK_ARENA_ATTN_FLOATS];
    float gate[NTK_ARENA_GATE_FLOATS];   // the widest row the GEMV accepts
};
__device__ __attribute__((aligned(256))) DecodeArena g_decode_arena;
template <int XS> struct XSlot { static constexpr int IN = XS == XS_GATE ? 14336 : 4096; };
template <int XS> __device__ __forceinline__ const float* xslot_ptr() {
    return XS == XS_HIDDEN ? g_decode_arena.hidden : XS == XS_ATTN ? g_decode_arena.attn_out : g_decode_arena.gate;
}

template <int DT, bool NORM, bool XFAST, bool A16, bool XI = false, bool LM = false, int NSF = NS_ANY, int XS = XS_NONE>
__device__ __forceinline__ void gemv_quant_body(const GemvParams& p, const int bid, const int nblk) {   // workgroup bid of nblk
    using F = Fmt<DT>;
    static_assert(!LM || (DT == NTK_DT_Q8_0 && !A16 && !XI), "lane-major rows: Q8_0");
    static_assert(NSF == NS_ANY || LM, "compile-time slice forms: the lane-major kernels");
    static_assert(XS == XS_NONE || (LM && XFAST && NSF != NS_ANY), "early-x forms: the lane-major kernels, fast prologue");
    constexpr int NL = LM ? 4 : F::NL;
    constexpr int STAGE = LM ? 0 : NL * 1024 + 64;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
#ifdef NTK_GEMV_TRACE
    unsigned long long gv_t[GT_EV] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#endif
    GV_STAMP(0);   // entry
#ifndef NTK_GEMV_NO_KARG_PREFETCH
    // The kernel arguments are 5 cache lines; hipcc fetches them piecemeal, each piece right before its first use, so the
    // prologue used to pay a scalar-cache miss per line one after the other before the first weight row could be requested.
    // Touch every line at once: the later loads hit the scalar cache.
    const auto* ka = __builtin_amdgcn_kernarg_segment_ptr();
    unsigned d0, d1, d2, d3, d4;
    if constexpr (XS == XS_NONE) {
        asm volatile("s_load_dword %0, %5, 0x0\n\ts_load_dword %1, %5, 0x40\n\ts_load_dword %2, %5, 0x80\n\ts_load_dword %3, %5, 0xc0\n\t"
                     "s_load_dword %4, %5, 0x100\n\ts_waitcnt lgkmcnt(0)"
                     : "=&s"(d0), "=&s"(d1), "=&s"(d2), "=&s"(d3), "=&s"(d4) : "s"(ka) : "memory");
    } else {   // early x: the wait stands behind the x requests below
        asm volatile("s_load_dword %0, %5, 0x0\n\ts_load_dword %1, %5, 0x40\n\ts_load_dword %2, %5, 0x80\n\ts_load_dword %3, %5, 0xc0\n\t"
                     "s_load_dword %4, %5, 0x100"
                     : "=&s"(d0), "=&s"(d1), "=&s"(d2), "=&s"(d3), "=&s"(d4) : "s"(ka) : "memory");
    }
    __builtin_amdgcn_sched_barrier(0);   // ... before the compiler's own argument loads
#endif

    const int tid = threadIdx.x;
    // The activations (and the norm weights) are requested before anything else is computed (fast prologue, see below): the row
    // bookkeeping that follows runs under their latency.  Register quads past the row's end are skipped by a uniform branch
    // (4096 columns use 2 of the 8; the dead loads alone cost 4 % of the token: they queue in front of the first weight row).
    constexpr int XIT = 8, WIT = 4;
    u32x4 xv[XIT], wv[WIT];
    if constexpr (XS != XS_NONE) {
        // x from its static slot: the same per-thread quads and the same clamping as below, with `in` and the thread count (512) known at
        // compile time -- nothing here reads an argument, so the requests fly beside the argument lines
        constexpr int IN = XSlot<XS>::IN, step0 = 512 * 4;
        const float* const xs = xslot_ptr<XS>();
#pragma unroll
        for (int i = 0; i < XIT; ++i) {
            xv[i] = u32x4{0u, 0u, 0u, 0u};
            if (i * step0 < IN) xv[i] = *reinterpret_cast<const u32x4*>(xs + min(tid * 4 + i * step0, IN - 4));
        }
        GV_STAMP(7);   // x requested
        __builtin_amdgcn_sched_barrier(0);
#ifndef NTK_GEMV_NO_KARG_PREFETCH
        // the argument lines have landed; the registers of the five loads stay reserved up to here
        asm volatile("s_waitcnt lgkmcnt(0)" : "+s"(d0), "+s"(d1), "+s"(d2), "+s"(d3), "+s"(d4) : : "memory");
        __builtin_amdgcn_sched_barrier(0);
#endif
        if constexpr (NORM) {   // (the norm weights' address is an argument)
#pragma unroll
            for (int i = 0; i < WIT; ++i) {
                wv[i] = u32x4{0u, 0u, 0u, 0u};
                if (i * step0 < IN) wv[i] = *reinterpret_cast<const u32x4*>(p.norm_w + min(tid * 4 + i * step0, IN - 4));
            }
        }
    } else
    if constexpr (XFAST) {
        const int step0 = (int)blockDim.x * 4;
#pragma unroll
        for (int i = 0; i < XIT; ++i) {
            xv[i] = u32x4{0u, 0u, 0u, 0u};
            if (i * step0 < p.in) xv[i] = *reinterpret_cast<const u32x4*>(p.x + min(tid * 4 + i * step0, p.in - 4));
        }
        if constexpr (NORM) {
#pragma unroll
            for (int i = 0; i < WIT; ++i) {
                wv[i] = u32x4{0u, 0u, 0u, 0u};
                if (i * step0 < p.in) wv[i] = *reinterpret_cast<const u32x4*>(p.norm_w + min(tid * 4 + i * step0, p.in - 4));
            }
        }
        GV_STAMP(7);   // x requested
    }
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ns = NSF == NS_ONE ? 1 : p.ns;
    const bool single = NSF == NS_ANY ? p.ns == 1 : NSF == NS_ONE;   // rows of one slice
    const int nwaves = ns * p.rw;
    const int s = wave % ns;        // column slice of this wave
    const int g = wave / ns;        // row group of this wave
    constexpr bool norm = NORM;   // compile-time: the norm-weight loads/stores must not sit behind a runtime branch

    // LDS: [activation image][per-wave staging of row bytes][partials].  Single-slice rows (<= 4096 columns) keep the image and
    // the staging areas apart, so a wave enters the row loop as soon as it has read its own activations; wider rows (image 35-70 KB)
    // reuse the image as staging area behind one more barrier.
    const size_t image_bytes = (size_t)std::min(ns, 4) * 64 * XPITCH * 4;
    const size_t stage0 = single ? image_bytes : 0;
    const size_t regionA = single ? image_bytes + (size_t)nwaves * STAGE : std::max((size_t)nwaves * STAGE, image_bytes);
    float* part = reinterpret_cast<float*>(smem + regionA);
    float* red = part + 2 * p.rw * ns * RB;
    const size_t lds_floats_total = regionA / 4 + (size_t)(2 * p.rw * ns * RB + 16 + 16);   // ... + red[16] + 16 spare

    // ---- item bookkeeping + first prefetch (issued before the prologue so HBM latency overlaps it) ----
    uint8_t* stage = smem + stage0 + (size_t)wave * STAGE;
    const int my_len = min(p.slice_cols, p.in - s * p.slice_cols);
    const int ncols = min(64, max(0, my_len - 64 * lane));
    const unsigned slice_byte0 = (unsigned)((size_t)s * p.slice_cols / F::BW * F::BB);
    const unsigned slice_bytes = (unsigned)(my_len / F::BW * F::BB);
    const int group = bid * p.rw + g;
    const int ngroups = nblk * p.rw;
    const int mats = p.silu_pair ? 2 : 1;
    const int n_my = (p.total_rows > group) ? ((p.total_rows - 1 - group) / ngroups + 1) * mats : 0;

    // item q of this wave -> (segment, row inside the segment); q < n_my  (per-lane form, used by the combine step)
    // The segment table of that step lives in scalar registers (MAX_SEG = 3: two row counts, three y pointers): a lane-indexed p.seg[seg] is a
    // dependent memory round trip at the end of every batch.  One segment: the target is segment 0, nothing to search.
    static_assert(MAX_SEG == 3, "locate / seg_y: unrolled for three segments");
    const int seg_rows0 = p.seg[0].rows, seg_rows1 = p.seg[1].rows;
    float* const seg_y0 = p.seg[0].y;
    float* const seg_y1 = p.seg[1].y;
    float* const seg_y2 = p.seg[2].y;
    auto locate = [&](int q, int& seg, int& row) {
        int r = group + (q >> (mats - 1)) * ngroups;   // mats is 1 or 2
        if (p.silu_pair) { seg = q & 1; row = r; return; }
        seg = 0;
        if (p.nseg > 1 && r >= seg_rows0) {
            r -= seg_rows0; seg = 1;
            if (p.nseg > 2 && r >= seg_rows1) { r -= seg_rows1; seg = 2; }
        }
        row = r;
    };
    auto seg_y = [&](int seg) { return seg == 0 ? seg_y0 : seg == 1 ? seg_y1 : seg_y2; };
    // The wave walks its items in order, so the location is kept as a cursor (scalar registers) and advanced
    // incrementally: one add and one compare per row instead of a search through the segment table.
    int cu_seg = 0, cu_row = group, cu_rows = p.silu_pair ? 0x7fffffff : p.seg[0].rows;   // cursor = next item to issue
    auto cursor_normalise = [&]() {
        while (cu_seg + 1 < p.nseg && cu_row >= cu_rows) { cu_row -= cu_rows; ++cu_seg; cu_rows = p.seg[cu_seg].rows; }
    };
    if (!p.silu_pair) cursor_normalise();
    auto cursor_advance = [&]() {
        if (p.silu_pair) {
            if (cu_seg == 0) { cu_seg = 1; } else { cu_seg = 0; cu_row += ngroups; }
        } else {
            cu_row += ngroups;
            cursor_normalise();
        }
    };

    u32x4 pf[NL], pf2[LM ? NL : 1];   // (LM: two register sets, rows alternate between them -- the prefetch of row q + 1 must not land on row q)
    uint32_t pf_sc = 0u, pf2_sc = 0u;   // LM: the lane's two FP16 scales
    // LM: lanes past the slice's end repeat its last lane (their activations are zero)
    const int lm_nl = my_len >> 6, lm_lane = min(lane, max(lm_nl - 1, 0));
    // rows that start 16-byte aligned (A16) cover the same 16-byte chunks row after row: the clamped chunk offsets are lane constants
    unsigned pre_off[NL];
    if constexpr (A16) {
        const unsigned last0 = (slice_bytes - 1u) & ~15u;
#pragma unroll
        for (int j = 0; j < NL; ++j) pre_off[j] = min(16u * (unsigned)(lane + 64 * j), last0);
    }
    int pf_seg = 0, pf_row = 0, pf_shift = 0;   // what the bytes in pf[] belong to
    float pf_res = 0.0f;                         // residual of that row (ns == 1): fetched a row ahead, not in the epilogue
    auto issue = [&]() {   // prefetch the item under the cursor (rows * row_bytes < 4 GiB: checked on the host)
        pf_seg = cu_seg; pf_row = cu_row;
        if (p.resid != nullptr && single) {
            int idx = cu_row;
            asm volatile("" : "+v"(idx));   // a vector load: a scalar one would sit in lgkmcnt in front of the LDS reads
            pf_res = p.resid[idx];
        }
        if constexpr (LM) return;   // (rows go through issue_lm)
        const unsigned rel = (unsigned)p.seg[cu_seg].delta + (unsigned)cu_row * p.row_bytes + slice_byte0;
        pf_shift = (int)(rel & 15u);
        const unsigned nbytes = (rel & 15u) + slice_bytes;
        const unsigned last = (nbytes - 1u) & ~15u;
        const uint8_t* a = p.seg[cu_seg].W + (rel & ~15u);
#pragma unroll
        for (int j = 0; j < NL; ++j) {
            unsigned off;
            if constexpr (A16) off = pre_off[j]; else off = min(16u * (unsigned)(lane + 64 * j), last);
            pf[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a + off));
        }
    };
    auto issue_lm = [&](u32x4 (&c)[NL], uint32_t& sc) {   // LM: the same item into the register set (c, sc); host: W 16-byte aligned (delta == 0)
        const uint8_t* a = p.seg[cu_seg].W + ((unsigned)cu_row * p.row_bytes + slice_byte0);
#pragma unroll
        for (int j = 0; j < NL; ++j)
            c[j] = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(a + 16u * (unsigned)(j * lm_nl + lm_lane)));
        sc = __builtin_nontemporal_load(reinterpret_cast<const uint32_t*>(a + 64u * (unsigned)lm_nl + 4u * (unsigned)lm_lane));
    };
    auto issue_first = [&]() { issue(); if constexpr (LM) issue_lm(pf, pf_sc); };
    if (n_my <= 0) { cu_seg = 0; cu_row = 0; }   // a wave without rows still prefetches (row 0): keeps the prologue branch-free

    // ---- prologue: this lane's 64 activations into registers (through a padded LDS image: coalesced
    //      global reads, conflict-free ds_read_b128), optional RMSNorm (reference rmsnorm.cu:16-70) ----
    f32x2 x2[32];   // the lane's 64 activations as 32 (even, odd) pairs
    XInt xi;         // ... or (XI) as integer byte planes (gemv_core.hip.h)
    static_assert(!XI || (XFAST && ((DT == NTK_DT_Q4_K && A16) || DT == NTK_DT_Q6_K)), "integer activations: fast prologue, Q4_K (aligned rows) / Q6_K");
    {
        // The activations reach registers through a padded LDS image holding ALL slices: image row (sp*64 + l)
        // = the 64 columns lane l of slice sp owns (pitch 68 floats: conflict-free ds_read_b128).
        //   * x (and the norm weights) are requested, and have landed, BEFORE the first weight prefetch: a CU serves its
        //     memory requests roughly in order, and x queued behind weight rows comes back with their HBM latency (see below);
        //   * RMSNorm is applied by the thread that loaded the element (x * rms_inv * w, rmsnorm.cu:68) and the
        //     image holds normalised values: the transposing read needs no second image and no extra registers
        //     (a weight image made hipcc spill the in-flight prefetch registers to scratch).
        float* ximg = reinterpret_cast<float*>(smem);
        constexpr int GS = 4;   // slices per image pass: 28672-wide rows (7 slices) take two passes, keeping LDS at 68 KB
        auto img_index = [&](int c, int g0) {
            if (single) return (c >> 6) * XPITCH + (c & 63);   // (uniform; spares the division)
            const int sp = c / p.slice_cols, cc = c - sp * p.slice_cols;
            return ((sp - g0) * 64 + (cc >> 6)) * XPITCH + (cc & 63);
        };
        const int step = (int)blockDim.x * 4;
        const int dummy = (int)(lds_floats_total - 16);   // 16 spare floats at the end of the allocation
        const bool have_lo = ncols > 0, have_hi = ncols > 32;   // ncols is 0, 32 or 64: two masks, not 64 compares
        auto read_own_row = [&](int g0) {
            // image row r = the 64 columns [64r, 64r+64) of the slice.  A lane owns row `lane`, except for Q6_K where it
            // owns columns 32t + [0,32) of rows (lane & ~1) and (lane | 1) (see Dot<Q6_K>)
            const float* xrow = ximg + ((s - g0) * 64 + lane) * XPITCH;
            const float* xr0 = xrow, *xr1 = xrow + 32;
            if constexpr (DT == NTK_DT_Q6_K) {
                xr0 = ximg + ((s - g0) * 64 + (lane & ~1)) * XPITCH + 32 * (lane & 1);
                xr1 = xr0 + XPITCH;
            }
#pragma unroll
            for (int j = 0; j < 64; j += 4) {
                const float4 v = *reinterpret_cast<const float4*>((j < 32 ? xr0 : xr1 - 32) + j);
                const bool have = j < 32 ? have_lo : have_hi;
                x2[j / 2] = f32x2{have ? v.x : 0.0f, have ? v.y : 0.0f};
                x2[j / 2 + 1] = f32x2{have ? v.z : 0.0f, have ? v.w : 0.0f};
            }
        };
        if constexpr (XFAST) {   // host guarantees: x (and norm_w) 16-byte aligned, in % 4 == 0, (!NORM || in <= WIT * step)
            // x (and the norm weights) were requested at the top and have LANDED before the first weight row is requested: a CU
            // returns its loads in request order, so an x request queued behind weight rows (this wave's, or those of the waves of
            // the workgroup that started earlier) comes back with HBM latency, and the prologue's barrier waits for the slowest
            // wave (tools/gemv_trace.py: x landed 0.25 us after its request in wave 0, activations in registers 2 us later; round 1
            // had already moved a wave's own x request in front of its weights, worth 3 us per launch).  Ordinary loads: the empty
            // asm "uses" them, so the compiler's own wait sits in front of it.
            // (-DNTK_GEMV_NO_XWAIT, tuning experiments: the first row right behind the x requests.  The matrix-core GEMV gained 5 % end to
            //  end from dropping its wait, gemv_rp.hip; here every wave needs the whole workgroup's image.  Round 5, same-box A/B
            //  alternated three times: 8B Q8_0 553.6 -> 546.8 tok/s, Wo 5.6 -> 6.5 us -- the wait stays.  profiles/r05_ab_variants.txt)
#ifndef NTK_GEMV_NO_XWAIT
            asm volatile("" : "+v"(xv[0]), "+v"(xv[1]), "+v"(xv[2]), "+v"(xv[3]), "+v"(xv[4]), "+v"(xv[5]), "+v"(xv[6]), "+v"(xv[7]));
            // (early x: letting the first row go without the norm weights measured the same as waiting for them -- NEGATIVE_RESULTS 12)
            if constexpr (NORM) asm volatile("" : "+v"(wv[0]), "+v"(wv[1]), "+v"(wv[2]), "+v"(wv[3]));
#endif
            issue_first();   // unconditional (a wave without rows re-reads row 0)
            GV_STAMP(8);   // first weight row requested
            __builtin_amdgcn_sched_barrier(0);
            GV_STAMP(1);   // x (and the norm weights) have landed
            float rms_inv = 1.0f;
            if constexpr (NORM) {   // sum x^2 over the row: every column is loaded by exactly one thread (i < WIT covers the row)
                float ssq = 0.0f;
#pragma unroll
                for (int i = 0; i < WIT; ++i) {
                    const float m = (tid * 4 + i * step < p.in) ? 1.0f : 0.0f;
                    const float x0 = __uint_as_float(xv[i].x), x1 = __uint_as_float(xv[i].y), x2_ = __uint_as_float(xv[i].z), x3 = __uint_as_float(xv[i].w);
                    ssq = fmaf(x0 * m, x0, ssq); ssq = fmaf(x1 * m, x1, ssq); ssq = fmaf(x2_ * m, x2_, ssq); ssq = fmaf(x3 * m, x3, ssq);
                }
                ssq = wave_sum(ssq);
                if (lane == 0) red[wave] = ssq;
                __syncthreads();
                float tot = 0.0f;
                for (int w = 0; w < nwaves; ++w) tot += red[w];
                rms_inv = 1.0f / sqrtf(tot / (float)p.in + p.eps);   // rsqrtf(mean + eps), rmsnorm.cu:60-61
#pragma unroll
                for (int i = 0; i < WIT; ++i) {   // x * rms_inv * w, the reference's association (rmsnorm.cu:68)
                    xv[i].x = __float_as_uint(__uint_as_float(xv[i].x) * rms_inv * __uint_as_float(wv[i].x));
                    xv[i].y = __float_as_uint(__uint_as_float(xv[i].y) * rms_inv * __uint_as_float(wv[i].y));
                    xv[i].z = __float_as_uint(__uint_as_float(xv[i].z) * rms_inv * __uint_as_float(wv[i].z));
                    xv[i].w = __float_as_uint(__uint_as_float(xv[i].w) * rms_inv * __uint_as_float(wv[i].w));
                }
            }
            if constexpr (XI) {
                // Integer planes instead of floats.  Image row (same 272-byte pitch as the float image: conflict-free b128 reads) =
                // [plane 0: 64 B][plane 1][plane 2][2^(e-22) of the row's two 32-column groups, the sums of x of its four 16-column
                // runs].  A thread converts 4 consecutive columns, 8 consecutive threads hold a 32-column sub-block: its exponent and
                // sum come from three DPP steps (every caller below keeps those 8 threads together: column bases are multiples of 256).
                uint8_t* dimg = smem;
                auto xi_store = [&](const u32x4 q, const int sp, const int cc, const bool live) {   // columns cc.. of slice sp
                    const float v0 = live ? __uint_as_float(q.x) : 0.0f, v1 = live ? __uint_as_float(q.y) : 0.0f,
                                v2 = live ? __uint_as_float(q.z) : 0.0f, v3 = live ? __uint_as_float(q.w) : 0.0f;
                    float am = fmaxf(fmaxf(fabsf(v0), fabsf(v1)), fmaxf(fabsf(v2), fabsf(v3)));
                    am = fmaxf(am, dpp_or_self<DPP_QUAD_1032, 0xF>(am));
                    am = fmaxf(am, dpp_or_self<DPP_QUAD_2301, 0xF>(am));
                    am = fmaxf(am, dpp_or_self<DPP_ROW_HALF_MIRROR, 0xF>(am));
                    float sm = (v0 + v1) + (v2 + v3);   // -> sum of the 16-column run (the thread's quad of lanes)
                    sm += dpp_or_zero<DPP_QUAD_1032, 0xF>(sm);
                    sm += dpp_or_zero<DPP_QUAD_2301, 0xF>(sm);
                    const int e = am > 0.0f ? __builtin_amdgcn_frexp_expf(am) : 0;   // am = m * 2^e, 0.5 <= m < 1
                    const float up = __builtin_ldexpf(1.0f, 22 - e), inv = __builtin_ldexpf(1.0f, e - 22);
                    // rint through the magic constant 1.5 * 2^23: the low mantissa bits ARE the two's-complement integer
                    const uint32_t x0 = __float_as_uint(fmaf(v0, up, 12582912.0f)) - 0x4B400000u, x1 = __float_as_uint(fmaf(v1, up, 12582912.0f)) - 0x4B400000u,
                                   x2i = __float_as_uint(fmaf(v2, up, 12582912.0f)) - 0x4B400000u, x3 = __float_as_uint(fmaf(v3, up, 12582912.0f)) - 0x4B400000u;
                    // 4 x 3 byte transpose: planes of the four columns
                    const uint32_t ta = __builtin_amdgcn_perm(x1, x0, 0x05010400u);    // x0.b0 x1.b0 x0.b1 x1.b1
                    const uint32_t tb = __builtin_amdgcn_perm(x1, x0, 0x07030602u);    // x0.b2 x1.b2 x0.b3 x1.b3
                    const uint32_t tc = __builtin_amdgcn_perm(x3, x2i, 0x05010400u);
                    const uint32_t td = __builtin_amdgcn_perm(x3, x2i, 0x07030602u);
                    const uint32_t p0 = __builtin_amdgcn_perm(tc, ta, 0x05040100u);    // b0 of columns 0..3
                    const uint32_t p1 = __builtin_amdgcn_perm(tc, ta, 0x07060302u);    // b1
                    const uint32_t p2 = __builtin_amdgcn_perm(td, tb, 0x05040100u);    // b2 (signed top byte)
                    if (live) {
                        uint8_t* row = dimg + (size_t)(sp * 64 + (cc >> 6)) * (XPITCH * 4);
                        *reinterpret_cast<uint32_t*>(row + (cc & 63)) = p0;
                        *reinterpret_cast<uint32_t*>(row + 64 + (cc & 63)) = p1;
                        *reinterpret_cast<uint32_t*>(row + 128 + (cc & 63)) = p2;
                        float* meta = reinterpret_cast<float*>(row + 192);   // [2^(e-22) x 2][run sums x 4]
                        if ((cc & 31) == 0) meta[(cc >> 5) & 1] = inv;          // first thread of the 32-column group
                        if ((cc & 15) == 0) meta[2 + ((cc >> 4) & 3)] = sm;     // first thread of the 16-column run
                    }
                };
                auto xi_read = [&](const int g0) {
                    // a lane's two 32-column groups: Q4_K -- both halves of image row `lane`; Q6_K -- half t of rows (lane & ~1) and
                    // (lane | 1) (columns 32 t + [0, 32) of each: see Dot<Q6_K>)
                    const bool have_lo_ = ncols > 0, have_hi_ = ncols > 32;
                    const uint8_t* rowA = dimg + (size_t)((s - g0) * 64 + lane) * (XPITCH * 4);
                    const uint8_t* rowB = rowA;
                    int offA = 0, offB = 32;
                    if constexpr (DT == NTK_DT_Q6_K) {
                        rowA = dimg + (size_t)((s - g0) * 64 + (lane & ~1)) * (XPITCH * 4);
                        rowB = rowA + XPITCH * 4;
                        offA = offB = 32 * (lane & 1);
                    }
#pragma unroll
                    for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                        for (int k4 = 0; k4 < 4; ++k4) {
                            const uint8_t* src = (k4 < 2 ? rowA + offA : rowB + offB) + 64 * pl + 16 * (k4 & 1);
                            const u32x4 v = *reinterpret_cast<const u32x4*>(src);
                            const bool have = k4 < 2 ? have_lo_ : have_hi_;
                            xi.d[pl][4 * k4] = have ? v.x : 0u; xi.d[pl][4 * k4 + 1] = have ? v.y : 0u;
                            xi.d[pl][4 * k4 + 2] = have ? v.z : 0u; xi.d[pl][4 * k4 + 3] = have ? v.w : 0u;
                        }
                    const float* mA = reinterpret_cast<const float*>(rowA + 192);
                    const float* mB = reinterpret_cast<const float*>(rowB + 192);
                    xi.inv[0] = have_lo_ ? mA[offA >> 5] : 0.0f;
                    xi.inv[1] = have_hi_ ? mB[offB >> 5] : 0.0f;
                    xi.sx[0] = have_lo_ ? mA[2 + (offA >> 4)] : 0.0f; xi.sx[1] = have_lo_ ? mA[3 + (offA >> 4)] : 0.0f;
                    xi.sx[2] = have_hi_ ? mB[2 + (offB >> 4)] : 0.0f; xi.sx[3] = have_hi_ ? mB[3 + (offB >> 4)] : 0.0f;
                };
                // (host: in <= XIT * step and ns <= 2, so the register quads cover the row and one image pass holds it.  Rows of
                // several slices -- the 14336 / 28672-column down projections -- were tried with a second pass from memory: correct,
                // and slower than the float form, 70B Q4_K down 33.4 -> 37.1 us: a workgroup converts the whole row for only 16 rows)
                int isp = 0, icc = tid * 4;   // (slice, column in the slice) of the thread's quad, advanced without a division: step < slice_cols
#pragma unroll
                for (int i = 0; i < XIT; ++i) {
                    if (i * step >= p.in) continue;   // uniform
                    xi_store(xv[i], isp, icc, tid * 4 + i * step < p.in);
                    icc += step;
                    if (icc >= p.slice_cols) { icc -= p.slice_cols; ++isp; }
                }
                __syncthreads();
                xi_read(0);
            } else
            {   // pass 0 (the only one up to 16384 columns): straight-line, the registers die here
                const int cend = min(p.in, GS * p.slice_cols);
                int isp = 0, icc = tid * 4;   // (slice, column in the slice) of the thread's quad, advanced without a division: step < slice_cols
#pragma unroll
                for (int i = 0; i < XIT; ++i) {
                    if (i * step >= cend) continue;   // uniform
                    const int c = tid * 4 + i * step;
                    *reinterpret_cast<u32x4*>(ximg + (c < cend ? (isp * 64 + (icc >> 6)) * XPITCH + (icc & 63) : dummy)) = xv[i];
                    icc += step;
                    if (icc >= p.slice_cols) { icc -= p.slice_cols; ++isp; }
                }
                for (int c = XIT * step + tid * 4; c < cend; c += step)   // columns the registers do not cover
                    *reinterpret_cast<float4*>(ximg + img_index(c, 0)) = *reinterpret_cast<const float4*>(p.x + c);
                GV_STAMP(9);    // image stores issued
                __syncthreads();
                GV_STAMP(10);   // image complete (barrier)
                if (s < GS) read_own_row(0);
#ifdef NTK_GEMV_TRACE
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                GV_STAMP(11);   // own row read
#endif
            }
            if constexpr (!XI)
            for (int g0 = GS; g0 < ns; g0 += GS) {   // 28672-wide rows: slices 4..6 in a second pass (weights already in flight)
                const int cbeg = g0 * p.slice_cols, cend = min(p.in, (g0 + GS) * p.slice_cols);
                __syncthreads();   // the previous pass has been read
                for (int c = cbeg + tid * 4; c < cend; c += step)
                    *reinterpret_cast<float4*>(ximg + img_index(c, g0)) = *reinterpret_cast<const float4*>(p.x + c);
                __syncthreads();
                if (s >= g0 && s < g0 + GS) read_own_row(g0);
            }
        } else {   // unaligned / odd sizes (and the NTK_GEMV_ABLATE=1 experiment): plain loops
            issue_first();
            float rms_inv = 1.0f;
            if (NORM && !(kAblate & 1)) {
                float ssq = 0.0f;
                for (int c = tid; c < p.in; c += blockDim.x) ssq = fmaf(p.x[c], p.x[c], ssq);
                ssq = wave_sum(ssq);
                if (lane == 0) red[wave] = ssq;
                __syncthreads();
                float tot = 0.0f;
                for (int w = 0; w < nwaves; ++w) tot += red[w];
                rms_inv = 1.0f / sqrtf(tot / (float)p.in + p.eps);
            }
            for (int g0 = 0; g0 < ns; g0 += GS) {
                const int cbeg = g0 * p.slice_cols, cend = min(p.in, (g0 + GS) * p.slice_cols);
                if (g0 > 0) __syncthreads();
                if (!(kAblate & 1)) {
                    for (int c = cbeg + tid; c < cend; c += blockDim.x)
                        ximg[img_index(c, g0)] = NORM ? p.x[c] * rms_inv * p.norm_w[c] : p.x[c];
                }
                __syncthreads();
                if (s >= g0 && s < g0 + GS) read_own_row(g0);
            }
        }
        if ((kAblate & 1) || XI) {   // (XI: x2 is not used; give the dead code below defined inputs)
#pragma unroll
            for (int j = 0; j < 32; ++j) x2[j] = f32x2{1.0f, 1.0f};
        }
        if (!single && !LM) __syncthreads();   // the image becomes the staging area
        GV_STAMP(2);   // activations in registers
    }
    float sx16[4], sx32[2];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        float t = 0.0f;
#pragma unroll
        for (int j = 0; j < 8; ++j) t += x2[8 * r + j].x + x2[8 * r + j].y;
        sx16[r] = t;
    }
    sx32[0] = sx16[0] + sx16[1];
    sx32[1] = sx16[2] + sx16[3];
    // 4-bit formats: the high nibbles are used in place (byte value 16 n, one v_and instead of shift + and), so the
    // activations of those columns carry the factor 1/16 -- a power of two: every product and sum is unchanged
    if constexpr (DT == NTK_DT_Q4_K) {
#pragma unroll
        for (int j = 16; j < 32; ++j) x2[j] *= 0.0625f;
    }
    if constexpr (DT == NTK_DT_Q4_0) {
#pragma unroll
        for (int j = 0; j < 32; ++j) if ((j & 8) != 0) x2[j] *= 0.0625f;   // pairs 8..15 of each 16: columns 16..31 of a block
    }
    float gate_carry = 0.0f;
    // SiLU(gate) * up epilogue of rows of one column slice: the wave's results are collected lane by lane (lane i keeps pair i of the
    // current batch of 64 pairs) and SiLU -- expf and a division, ~25 VALU instructions -- runs ONCE per batch on up to 64 lanes instead
    // of once per pair on one lane (the K-quant launches are VALU-issue bound: 12 of ~145 instructions per row went here)
    float pair_g = 0.0f, pair_u = 0.0f;
    auto silu_flush = [&](const int last_pair) {   // pairs (last_pair & ~63) .. last_pair of this wave
        const int base = last_pair & ~63;
        if (lane <= last_pair - base) {
            const int row = group + (base + lane) * ngroups;
            p.seg[0].y[row] = pair_g / (1.0f + expf(-pair_g)) * pair_u;   // reference gemm.cu:719-724
        }
    };

    // cross-slice combine of one batch (ns > 1): wave s == 0 of each row group sums the ns partials of
    // item i in slice order and applies the epilogue; `cnt` items of batch b are valid
    float res_pf = 0.0f;
    auto prefetch_resid = [&](int b) {   // ns > 1: the combining wave fetches batch b's residuals one batch ahead
        if (p.resid == nullptr || s != 0 || lane >= RB || b * RB + lane >= n_my) return;
        int seg, row;
        locate(b * RB + lane, seg, row);
        res_pf = p.resid[row];
    };
    if (!single) prefetch_resid(0);
    auto combine = [&](int b, int cnt) {
        if (s != 0) return;
        const float* pg = part + (size_t)(b & 1) * p.rw * ns * RB + (size_t)(g * ns) * RB;
        float t = 0.0f;
        if (lane < cnt)
            for (int ss = 0; ss < ns; ++ss) t += pg[ss * RB + lane];
        const float nxt = __shfl_down(t, 1, 64);
        if (lane < cnt) {
            int seg, row;
            locate(b * RB + lane, seg, row);
            if (p.silu_pair) {
                if ((lane & 1) == 0) seg_y0[row] = t / (1.0f + expf(-t)) * nxt;
            } else {
                float v = t;
                if (p.resid != nullptr && seg == 0) v = res_pf + v;
                seg_y(seg)[row] = v;
            }
        }
        prefetch_resid(b + 1);
    };

    // ---- row streaming ---------------------------------------------------------------------------
    // Every wave walks its own list of (segment,row) items; the valid ones are a prefix of length n_my.
    // All loads / LDS writes are unpredicated (lanes past the slice end re-read its last chunk) so the loop
    // body is straight-line code: hipcc then waits for the prefetch exactly once, right before the ds_writes.
    // One row: `cur` (LM) holds its bytes, the next row's go to `nxt`.
    auto row_step = [&](const int q, u32x4 (&cur)[NL], uint32_t& cur_sc, u32x4 (&nxt)[LM ? NL : 1], uint32_t& nxt_sc) __attribute__((always_inline)) {
        const int seg = pf_seg, row = pf_row, shift = A16 ? 0 : pf_shift;
        const float res = pf_res;
        float acc;
        if constexpr (LM) {
            // the row's registers are "used" here, so the wait for them stands in front of the next row's requests (as the ds_writes of the staged form)
            asm volatile("" : "+v"(cur[0]), "+v"(cur[1]), "+v"(cur[2]), "+v"(cur[3]), "+v"(cur_sc));
#ifdef NTK_GEMV_TRACE
            if (q == 0) GV_STAMP(3);            // first row has landed
            if (q == n_my - 1) GV_STAMP(5);     // last row has landed
#endif
            if (q + 1 < n_my) { cursor_advance(); issue(); issue_lm(nxt, nxt_sc); }   // next row's bytes fly while this one is decoded
            __builtin_amdgcn_sched_barrier(0);   // ... requested BEFORE the decode, not where the scheduler finds room
            acc = dot_q8_regs(cur, cur_sc, ncols, x2);
        } else {
#pragma unroll
            for (int j = 0; j < NL; ++j) {
                if (kAblate & 4) { asm volatile("" ::"v"(pf[j])); continue; }
                *reinterpret_cast<u32x4*>(stage + 16 * (lane + 64 * j)) = pf[j];
            }
            __builtin_amdgcn_wave_barrier();   // DS ops of one wave execute in order: the image is visible below
#ifdef NTK_GEMV_TRACE
            if (q == 0) GV_STAMP(3);            // first row has landed
            if (q == n_my - 1) GV_STAMP(5);     // last row has landed
#endif
            if (q + 1 < n_my) { cursor_advance(); issue(); }   // next row's bytes fly while this one is decoded
            if constexpr (XI && DT == NTK_DT_Q6_K) acc = DotI<DT>::run(stage, shift, lane, ncols, xi);
            else if constexpr (XI) acc = DotI<DT>::run(stage, lane, ncols, xi);
            else acc = (kAblate & 2) ? x2[0].x + (float)q : Dot<DT, A16>::run(stage, shift, lane, ncols, x2, sx16, sx32);
            __builtin_amdgcn_wave_barrier();   // all reads of the image precede the next overwrite
        }
        const float tot = wave_sum_lane63(acc);   // valid in lane 63
#ifdef NTK_GEMV_TRACE
        if (q == 0) { asm volatile("" :: "v"(tot)); GV_STAMP(4); }   // first row decoded and reduced
#endif

        if (single) {
            if (p.silu_pair) {
                const float t63 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tot), 63));
                const int pi = (q >> 1) & 63;
                if ((q & 1) == 0) { if (lane == pi) pair_g = t63; }
                else {
                    if (lane == pi) pair_u = t63;
                    if (pi == 63 || q == n_my - 1) silu_flush(q >> 1);   // n_my is even: gate and up rows alternate
                }
            } else if (lane == 63) {
                float v = tot;
                if (p.resid != nullptr && seg == 0) v = res + v;                      // reference elementwise.cu:23-32
                p.seg[seg].y[row] = v;
            }
        } else {
            const int b = q / RB, i = q % RB;
            if (lane == 63) part[(size_t)(b & 1) * p.rw * ns * RB + (size_t)(g * ns + s) * RB + i] = tot;
            if (i == RB - 1) {
                __syncthreads();
                combine(b, RB);
            }
        }
    };
    for (int q = 0; q < n_my; ++q) {
        row_step(q, pf, pf_sc, pf2, pf2_sc);
        if constexpr (LM) { if (++q < n_my) row_step(q, pf2, pf2_sc, pf, pf_sc); }
    }
    if (!single) {   // close a partial batch, then keep barrier counts equal across the workgroup
        int done = n_my / RB;
        if (n_my % RB) {
            __syncthreads();
            combine(done, n_my % RB);
            ++done;
        }
        for (; done < p.nbatch; ++done) __syncthreads();
    }
#ifdef NTK_GEMV_TRACE
    GV_STAMP(6);   // end
    if (tid == 0 && bid < GT_WG) {
        gv_t[13] = (unsigned long long)n_my;
        for (int e = 0; e < GT_EV; ++e) g_gemv_trace[p.trace_slot & (GT_SLOTS - 1)][bid][e] = gv_t[e];
    }
#endif
}

// Q8_0 rows in the lane-major layout of the engine's repack (LM above)
template <bool NORM, bool XFAST, int NSF, int XS = XS_NONE>
__global__ __launch_bounds__(512, Fmt<NTK_DT_Q8_0>::MINW) void gemv_q8l_kernel(const GemvParams p) {
    gemv_quant_body<NTK_DT_Q8_0, NORM, XFAST, false, false, true, NSF, XS>(p, (int)blockIdx.x, (int)gridDim.x);
}
// GGUF Q8_0 rows -> lane-major rows (UNPACK: back).  One thread per (row, 64-column lane): its two blocks are 17 dwords
// [d0 | 32 quants | d1 | 32 quants] in the file (4-byte aligned: the tensor is, and a row is a multiple of 272 bytes), 16 quant dwords + 1 scale dword packed.
template <bool UNPACK>
__global__ __launch_bounds__(256) void q8l_pack_kernel(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, const int rows, const int in,
                                                       const int slice_cols) {
    const int lanes_row = in >> 6;
    const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (size_t)rows * lanes_row) return;
    const int row = (int)(t / lanes_row), gl = (int)(t % lanes_row);       // gl: the lane's 64-column group in the row
    const int lanes_slice = slice_cols >> 6, sl = gl / lanes_slice, l = gl - sl * lanes_slice;
    const int nl = min(lanes_slice, lanes_row - sl * lanes_slice);          // lanes of this slice (the last one may be shorter)
    const size_t row0 = (size_t)row * lanes_row * 68;
    uint32_t* file = reinterpret_cast<uint32_t*>(const_cast<uint8_t*>(UNPACK ? dst : src) + row0 + (size_t)gl * 68);
    uint8_t* slice = const_cast<uint8_t*>(UNPACK ? src : dst) + row0 + (size_t)sl * lanes_slice * 68;
    uint32_t w[17], q[16], sc;
    if constexpr (!UNPACK) {
#pragma unroll
        for (int k = 0; k < 17; ++k) w[k] = file[k];
#pragma unroll
        for (int k = 0; k < 8; ++k) { q[k] = (w[k] >> 16) | (w[k + 1] << 16); q[8 + k] = w[9 + k]; }
        sc = (w[0] & 0xFFFFu) | (w[8] & 0xFFFF0000u);
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<u32x4*>(slice + (size_t)(j * nl + l) * 16) = u32x4{q[4 * j], q[4 * j + 1], q[4 * j + 2], q[4 * j + 3]};
        *reinterpret_cast<uint32_t*>(slice + (size_t)64 * nl + 4 * l) = sc;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(slice + (size_t)(j * nl + l) * 16);
            q[4 * j] = v.x; q[4 * j + 1] = v.y; q[4 * j + 2] = v.z; q[4 * j + 3] = v.w;
        }
        sc = *reinterpret_cast<const uint32_t*>(slice + (size_t)64 * nl + 4 * l);
        w[0] = (sc & 0xFFFFu) | (q[0] << 16);
#pragma unroll
        for (int k = 1; k < 8; ++k) w[k] = (q[k - 1] >> 16) | (q[k] << 16);
        w[8] = (q[7] >> 16) | (sc & 0xFFFF0000u);
#pragma unroll
        for (int k = 0; k < 8; ++k) w[9 + k] = q[8 + k];
#pragma unroll
        for (int k = 0; k < 17; ++k) file[k] = w[k];
    }
}

template <int DT, bool NORM, bool XFAST, bool A16>
__global__ __launch_bounds__(512, Fmt<DT>::MINW) void gemv_quant_kernel(const GemvParams p) {
    gemv_quant_body<DT, NORM, XFAST, A16>(p, (int)blockIdx.x, (int)gridDim.x);
}
// integer-activation form (Q4_K, aligned fast prologue, rows of <= 16384 columns): gemv_core.hip.h XInt / DotI
template <int DT, bool NORM>
__global__ __launch_bounds__(512, Fmt<DT>::MINW) void gemv_quant_xi_kernel(const GemvParams p) {
    gemv_quant_body<DT, NORM, true, A16_OK<DT>, true>(p, (int)blockIdx.x, (int)gridDim.x);
}
// Two weight formats in ONE launch (llama.cpp's Q4_K_M stores attn_v as Q6_K / Q5_K next to Q4_K attn_q / attn_k): the first
// `split` workgroups run format A on its segments, the rest format B on its own -- the two halves share nothing but x.  One
// launch instead of two for the fused norm + Q|K|V projection of those layers (16 of 32 at 8B, all 80 at 70B).
template <int DTA, int DTB, bool NORM>
__global__ __launch_bounds__(512, 4) void gemv_quant_pair_kernel(const GemvParams pa, const GemvParams pb, const int split) {
    if ((int)blockIdx.x < split) gemv_quant_body<DTA, NORM, true, A16_OK<DTA>>(pa, (int)blockIdx.x, split);
    else gemv_quant_body<DTB, NORM, true, A16_OK<DTB>>(pb, (int)blockIdx.x - split, (int)gridDim.x - split);
}

// ------------------------------------------------------------------------------------------------
// Dense F16 / BF16 / F32 rows (reference gemm.cu:476-671; BF: the 16-bit words are bfloat16, widened exactly by bits << 16): one wave per row,
// 16-byte lane loads when the row is aligned, scalar otherwise (the reference's own F32 test uses in = 3).  The 1:1 launcher: the engine's
// 16-bit models run on gemv_dense16.hip and come here only with dense_fused = 0 or with shapes that kernel does not take.
// ------------------------------------------------------------------------------------------------
template <bool BF> __device__ __forceinline__ float w16f(uint16_t bits) {
    if constexpr (BF) return __uint_as_float((uint32_t)bits << 16); else return h2f(bits);
}
template <typename T, bool ADD, bool BF = false>
__global__ __launch_bounds__(256) void gemv_dense_kernel(float* __restrict__ y, const T* __restrict__ W,
                                                         const float* __restrict__ x, int out, int in) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int nwaves = gridDim.x * (blockDim.x >> 6);
    constexpr int V = 16 / (int)sizeof(T);
    for (int r = wave; r < out; r += nwaves) {
        const T* w = W + (size_t)r * in;
        float acc = 0.0f;
        int done = 0;
        if ((reinterpret_cast<uintptr_t>(w) & 15) == 0 && (reinterpret_cast<uintptr_t>(x) & 15) == 0) {
            const int nv = in / V;
            for (int i = lane; i < nv; i += 64) {
                const u32x4 raw = __builtin_nontemporal_load(reinterpret_cast<const u32x4*>(w) + i);
                if constexpr (sizeof(T) == 4) {
                    const float4 xv = *reinterpret_cast<const float4*>(x + 4 * i);
                    acc = fmaf(__uint_as_float(raw.x), xv.x, acc); acc = fmaf(__uint_as_float(raw.y), xv.y, acc);
                    acc = fmaf(__uint_as_float(raw.z), xv.z, acc); acc = fmaf(__uint_as_float(raw.w), xv.w, acc);
                } else {
                    const float4 x0 = *reinterpret_cast<const float4*>(x + 8 * i);
                    const float4 x1 = *reinterpret_cast<const float4*>(x + 8 * i + 4);
                    acc = fmaf(w16f<BF>((uint16_t)(raw.x & 0xFFFF)), x0.x, acc); acc = fmaf(w16f<BF>((uint16_t)(raw.x >> 16)), x0.y, acc);
                    acc = fmaf(w16f<BF>((uint16_t)(raw.y & 0xFFFF)), x0.z, acc); acc = fmaf(w16f<BF>((uint16_t)(raw.y >> 16)), x0.w, acc);
                    acc = fmaf(w16f<BF>((uint16_t)(raw.z & 0xFFFF)), x1.x, acc); acc = fmaf(w16f<BF>((uint16_t)(raw.z >> 16)), x1.y, acc);
                    acc = fmaf(w16f<BF>((uint16_t)(raw.w & 0xFFFF)), x1.z, acc); acc = fmaf(w16f<BF>((uint16_t)(raw.w >> 16)), x1.w, acc);
                }
            }
            done = nv * V;
        }
        for (int i = done + lane; i < in; i += 64) {
            float wv;
            if constexpr (sizeof(T) == 4) wv = (float)w[i]; else wv = w16f<BF>((uint16_t)w[i]);
            acc = fmaf(wv, x[i], acc);
        }
        acc = wave_sum(acc);
        if (lane == 0) y[r] = ADD ? y[r] + acc : acc;
    }
}

// ------------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------------
static bool is_quant(int dt) {
    return dt == NTK_DT_Q8_0 || dt == NTK_DT_Q4_0 || dt == NTK_DT_Q4_K || dt == NTK_DT_Q5_K || dt == NTK_DT_Q6_K;
}

struct GemvLaunch {
    GemvParams p;
    int grid, nwaves;
    size_t lds;
    bool xfast, a16;
};

static bool raise_lds_limit(const void* fn) {
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
}

// argument checks + geometry of one single-format launch (max_wg workgroups at most)
template <int DT>
static int prepare_quant(const ntk_gemv_seg* segs, int nseg, const float* x, int in, const float* norm_w, float eps,
                         const float* resid, int silu_pair, int max_wg, GemvLaunch& L, bool lm = false) {
    using F = Fmt<DT>;
    if (in <= 0 || in % F::BW != 0) return NTK_E_SHAPE;
    GemvParams& p = L.p;
    p = GemvParams{};
    long total = 0;
    const size_t row_bytes = (size_t)in / F::BW * F::BB;
    for (int i = 0; i < nseg; ++i) {
        if (segs[i].rows < 0) return NTK_E_SHAPE;
        if (segs[i].rows > 0 && (!segs[i].W || !segs[i].y)) return NTK_E_NULL;
        if ((size_t)segs[i].rows * row_bytes > 0xFFFFFFF0ull) return NTK_E_SHAPE;
        const uintptr_t w = reinterpret_cast<uintptr_t>(segs[i].W);
        if (w & 1) return NTK_E_ALIGN;
        p.seg[i].W = reinterpret_cast<const uint8_t*>(w & ~(uintptr_t)15);
        p.seg[i].delta = (int)(w & 15);
        p.seg[i].y = segs[i].y;
        p.seg[i].rows = segs[i].rows;
        total += segs[i].rows;
    }
    if (silu_pair) {
        if (nseg != 2 || segs[0].rows != segs[1].rows || resid) return NTK_E_SHAPE;
        total = segs[0].rows;
    }
    p.nseg = nseg;
    p.total_rows = (int)total;
    p.x = x;
    p.in = in;
    if (!gemv_slices(in, F::BW == 256 ? 256 : 64, p.ns, p.slice_cols)) return NTK_E_SHAPE;
    // waves per workgroup = ns * rw ~ 8: one x prologue feeds eight row streams
    static const int env_waves = std::max(1, NTK_TUNE_ENV_INT("NTK_GEMV_WAVES", 8));   // (tuning builds only)
    p.rw = std::max(1, env_waves / p.ns);   // (6-wave workgroups for the 3-waves/SIMD formats measured 30 % slower)
    L.nwaves = p.ns * p.rw;
    p.x_vec = ((reinterpret_cast<uintptr_t>(x) & 15) == 0 &&
               (!norm_w || (reinterpret_cast<uintptr_t>(norm_w) & 15) == 0) && (p.slice_cols % 4 == 0)) ? 1 : 0;
    p.norm_w = norm_w;
    p.eps = eps;
    p.resid = resid;
    p.silu_pair = silu_pair;
    p.row_bytes = (unsigned)row_bytes;
    const int mats = silu_pair ? 2 : 1;
    // enough workgroups to fill 256 CUs twice over, but never more row groups than rows
    int grid = (int)std::min<long>((total + p.rw - 1) / p.rw, max_wg);
    grid = std::max(grid, 1);
    L.grid = grid;
    const long ngroups = (long)grid * p.rw;
    const long rows_per_group = (total + ngroups - 1) / ngroups;
    p.nbatch = (int)((rows_per_group * mats + RB - 1) / RB);
    const int STAGE = lm ? 0 : F::NL * 1024 + 64;   // (lane-major rows go to registers: no staging areas)
    const size_t image_bytes = (size_t)std::min(p.ns, 4) * 64 * XPITCH * 4;   // same layout as gemv_quant_body
    const size_t regionA = p.ns == 1 ? image_bytes + (size_t)L.nwaves * STAGE : std::max((size_t)L.nwaves * STAGE, image_bytes);
    L.lds = regionA + (size_t)(2 * p.rw * p.ns * RB + 16 + 16) * sizeof(float);
    // fast prologue: aligned x / norm weights, whole float4s, norm weights fit the 4 register slots per thread
    L.xfast = p.x_vec && (in % 4 == 0) && in >= 4 && !(kAblate & 1) && (!norm_w || in <= 4 * 4 * 64 * L.nwaves) &&
              (p.ns == 1 || 4 * 64 * L.nwaves <= p.slice_cols);   // (the image index advances by one thread-count step per register quad)
    // A16 (K-quants whose blocks are multiples of 16 bytes): every row slice starts 16-byte aligned -> b128 LDS reads,
    // no v_alignbyte.  True for every GGUF tensor (data offsets are 32-byte aligned); the general form covers the rest.
    bool a16 = (DT == NTK_DT_Q4_K || DT == NTK_DT_Q5_K);
    for (int i = 0; i < nseg; ++i) a16 = a16 && p.seg[i].delta == 0;
    L.a16 = a16;
    return NTK_OK;
}

// smallest launch (bytes of weights) that takes the integer-activation form of the Q4_K / Q6_K GEMV: 48 MiB (measured, section 3.1 of DESIGN.md:
// below it the conversion in the prologue costs what the decode saves).  A constant of the library; the parity tests reach the form on
// small launches through the per-call argument of ntk_debug_gemv_fused_form.
constexpr size_t kXiMinBytes = (size_t)48 << 20;
enum { XI_DEFAULT = -1, XI_NEVER = 0, XI_ALWAYS = 1 };

static int max_workgroups() {
    static const int max_wg = std::max(1, NTK_TUNE_ENV_INT("NTK_GEMV_MAX_WG", 512));   // (tuning builds only)
    return max_wg;
}

template <int DT>
static int launch_quant(const ntk_gemv_seg* segs, int nseg, const float* x, int in, const float* norm_w, float eps,
                        const float* resid, int silu_pair, hipStream_t st, int xi_mode = XI_DEFAULT) {
    GemvLaunch L;
    const int rc = prepare_quant<DT>(segs, nseg, x, in, norm_w, eps, resid, silu_pair, max_workgroups(), L);
    if (rc != NTK_OK) return rc;
    if (L.p.total_rows == 0) return NTK_OK;
    using KernelFn = void (*)(const GemvParams);
    static const KernelFn table[2][2][2] = {
        {{gemv_quant_kernel<DT, false, false, false>, gemv_quant_kernel<DT, false, false, A16_OK<DT>>},
         {gemv_quant_kernel<DT, false, true, false>, gemv_quant_kernel<DT, false, true, A16_OK<DT>>}},
        {{gemv_quant_kernel<DT, true, false, false>, gemv_quant_kernel<DT, true, false, A16_OK<DT>>},
         {gemv_quant_kernel<DT, true, true, false>, gemv_quant_kernel<DT, true, true, A16_OK<DT>>}}};
    if (L.lds > 64 * 1024) {   // 28672-wide rows: the activation image alone is 119 KiB
        static bool once = [] {
            bool ok = true;
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b)
                    for (int c = 0; c < 2; ++c)
                        ok = ok && hipFuncSetAttribute((const void*)table[a][b][c], hipFuncAttributeMaxDynamicSharedMemorySize,
                                                       160 * 1024) == hipSuccess;
            return ok;
        }();
        if (!once || L.lds > 160 * 1024) return NTK_E_SHAPE;
    }
    const dim3 g(L.grid), b(64 * L.nwaves);
#ifdef NTK_GEMV_TRACE
    static int trace_counter = 0;
    L.p.trace_slot = trace_counter++;
#endif
    if constexpr (DT == NTK_DT_Q4_K || DT == NTK_DT_Q6_K) {
        // the integer-activation form: registers of the fast prologue cover the row, one image pass
        // ... and only the launches that are VALU-bound gain: long ones (measured, tools/gemv_bench.py: 70B gate|up 53.0 -> 49.1 us,
        // Q4_K LM head 56.6 -> 54.0, 8B gate|up 20.0 -> 17.1-18.8; under ~48 MiB -- 70B Q|K|V, the 8B down projection -- nothing is
        // gained or the conversion in the prologue costs more than the decode saves)
        const size_t launch_bytes = (size_t)L.p.total_rows * (silu_pair ? 2 : 1) * L.p.row_bytes;
        const bool want = xi_mode == XI_ALWAYS || (xi_mode == XI_DEFAULT && launch_bytes >= kXiMinBytes);
        if (want && L.xfast && (L.a16 || DT == NTK_DT_Q6_K) && L.p.ns <= 2 && in <= 8 * 4 * 64 * L.nwaves) {
            using XFn = void (*)(const GemvParams);
            static const XFn xt[2] = {gemv_quant_xi_kernel<DT, false>, gemv_quant_xi_kernel<DT, true>};
            if (L.lds > 64 * 1024) {
                static bool once2 = hipFuncSetAttribute((const void*)xt[0], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
                                    hipFuncSetAttribute((const void*)xt[1], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
                if (!once2) return NTK_E_SHAPE;
            }
            hipLaunchKernelGGL(xt[norm_w ? 1 : 0], g, b, L.lds, st, L.p);
            return last_launch_status();
        }
    }
    hipLaunchKernelGGL(table[norm_w ? 1 : 0][L.xfast ? 1 : 0][L.a16 ? 1 : 0], g, b, L.lds, st, L.p);
    return last_launch_status();
}

// ---- lane-major Q8_0: size, pack / unpack (ntk_q8l_bytes / ntk_q8l_pack / ntk_q8l_unpack), launch (the all-Q8_0 side of ntk_gemv_rp_fused) ----
static size_t q8l_bytes(int rows, int in) {
    int ns, sc;
    return rows > 0 && q8l_layout(in, ns, sc) ? (size_t)rows * (size_t)(in / 32 * 34) : 0;
}

static int q8l_pack(void* dst, const void* raw, int rows, int in, bool unpack, hipStream_t st) {
    int ns, sc;
    if (rows <= 0 || !q8l_layout(in, ns, sc)) return NTK_E_SHAPE;
    // (dst: the packed side when packing, the GGUF side when unpacking)
    if ((reinterpret_cast<uintptr_t>(unpack ? raw : dst) & 15) || (reinterpret_cast<uintptr_t>(unpack ? dst : raw) & 3)) return NTK_E_ALIGN;
    const size_t n = (size_t)rows * (in / 64);
    if ((n + 255) / 256 > 0x7FFFFFFFull) return NTK_E_SHAPE;
    const dim3 g((unsigned)((n + 255) / 256)), b(256);
    uint8_t* d = static_cast<uint8_t*>(dst);
    const uint8_t* r = static_cast<const uint8_t*>(raw);
    if (unpack) hipLaunchKernelGGL(q8l_pack_kernel<true>, g, b, 0, st, d, r, rows, in, sc);
    else hipLaunchKernelGGL(q8l_pack_kernel<false>, g, b, 0, st, d, r, rows, in, sc);
    return last_launch_status();
}

// ---- the static decode activations: slot addresses per device (asked once, outside any stream capture), ownership ----
constexpr int kArenaDevices = 16;
struct ArenaDev {
    std::atomic<int> known{0};   // 1: addr[] is valid, -1: the lookup failed
    std::atomic<int> owned{0};
    const float* addr[4] = {nullptr, nullptr, nullptr, nullptr};   // [XS_*]
};
static ArenaDev g_arena_dev[kArenaDevices];
static std::mutex g_arena_mu;
static thread_local int t_last_static_x = XS_NONE;

static ArenaDev* arena_dev(bool lookup) {   // the current device's entry (lookup: resolve the symbol if nobody has)
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kArenaDevices) return nullptr;
    ArenaDev& a = g_arena_dev[dev];
    if (a.known.load(std::memory_order_acquire) == 0 && lookup) {
        std::lock_guard<std::mutex> lk(g_arena_mu);
        if (a.known.load(std::memory_order_relaxed) == 0) {
            void* base = nullptr;
            const bool ok = hipGetSymbolAddress(&base, HIP_SYMBOL(g_decode_arena)) == hipSuccess && base != nullptr;
            if (ok) {
                auto* f = static_cast<const float*>(base);
                a.addr[XS_HIDDEN] = f + offsetof(DecodeArena, hidden) / 4;
                a.addr[XS_ATTN] = f + offsetof(DecodeArena, attn_out) / 4;
                a.addr[XS_GATE] = f + offsetof(DecodeArena, gate) / 4;
            }
            a.known.store(ok ? 1 : -1, std::memory_order_release);
        }
    }
    return a.known.load(std::memory_order_acquire) == 1 ? &a : nullptr;
}
// the slot whose early-x form takes (x, in), or XS_NONE
static int static_x_slot(const float* x, int in) {
    const ArenaDev* a = arena_dev(false);
    if (!a) return XS_NONE;
    if (x == a->addr[XS_HIDDEN] && in == XSlot<XS_HIDDEN>::IN) return XS_HIDDEN;
    if (x == a->addr[XS_ATTN] && in == XSlot<XS_ATTN>::IN) return XS_ATTN;
    if (x == a->addr[XS_GATE] && in == XSlot<XS_GATE>::IN) return XS_GATE;
    return XS_NONE;
}

int q8l_gemv_fused(const ntk_gemv_seg* segs, int nseg, const float* x, int in, const float* norm_w, float eps, const float* resid,
                   int silu_pair, hipStream_t st) {
    int ns, sc;
    t_last_static_x = XS_NONE;
    if (!q8l_layout(in, ns, sc)) return NTK_E_SHAPE;
    for (int i = 0; i < nseg; ++i)
        if (reinterpret_cast<uintptr_t>(segs[i].W) & 15) return NTK_E_ALIGN;   // rows are read with 16-byte requests from the tensor's own start
    GemvLaunch L;
    const int rc = prepare_quant<NTK_DT_Q8_0>(segs, nseg, x, in, norm_w, eps, resid, silu_pair, max_workgroups(), L, true);
    if (rc != NTK_OK) return rc;
    if (L.p.total_rows == 0) return NTK_OK;
    using KernelFn = void (*)(const GemvParams);
#define Q8L_FORMS(NORM, XFAST) {gemv_q8l_kernel<NORM, XFAST, NS_ONE>, gemv_q8l_kernel<NORM, XFAST, NS_SPLIT>}
    static const KernelFn table[2][2][2] = {{Q8L_FORMS(false, false), Q8L_FORMS(false, true)}, {Q8L_FORMS(true, false), Q8L_FORMS(true, true)}};
#undef Q8L_FORMS
    if (L.lds > 64 * 1024) {   // 28672-wide rows: the activation image of four slices, 68 KiB
        static const bool once = [] {
            bool ok = true;
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b)
                    for (int c = 0; c < 2; ++c) ok = ok && raise_lds_limit((const void*)table[a][b][c]);
            return ok;
        }();
        if (!once || L.lds > 160 * 1024) return NTK_E_SHAPE;
    }
#ifdef NTK_GEMV_TRACE
    static int trace_counter = 0;
    L.p.trace_slot = trace_counter++;
#endif
    // x in a static slot (pointer identity), the slot's width, the fast prologue on 512 threads: the early-x form of the same kernel
    KernelFn fn = table[norm_w ? 1 : 0][L.xfast ? 1 : 0][L.p.ns == 1 ? 0 : 1];
    if (L.xfast && L.nwaves == 8) {
        const int xs = static_x_slot(x, in);
        KernelFn early = nullptr;
        if (xs == XS_HIDDEN && L.p.ns == 1 && norm_w) early = gemv_q8l_kernel<true, true, NS_ONE, XS_HIDDEN>;   // (every reader of the hidden state norms it)
        else if (xs == XS_ATTN && L.p.ns == 1 && !norm_w) early = gemv_q8l_kernel<false, true, NS_ONE, XS_ATTN>;
        else if (xs == XS_GATE && L.p.ns > 1 && !norm_w) {   // (14336 columns: the activation image of four slices, 68 KiB)
            static const bool raised = raise_lds_limit((const void*)gemv_q8l_kernel<false, true, NS_SPLIT, XS_GATE>);
            if (raised || L.lds <= 64 * 1024) early = gemv_q8l_kernel<false, true, NS_SPLIT, XS_GATE>;
        }
        if (early && L.lds <= 160 * 1024) { fn = early; t_last_static_x = xs; }
    }
    hipLaunchKernelGGL(fn, dim3(L.grid), dim3(64 * L.nwaves), L.lds, st, L.p);
    return last_launch_status();
}


// segments of two formats sharing x (no residual / SiLU epilogue): one launch, workgroups split by bytes
template <int DTA, int DTB>
static int launch_pair(const ntk_gemv_seg* sa, int na, const ntk_gemv_seg* sb, int nb, const float* x, int in, const float* norm_w,
                       float eps, hipStream_t st) {
    const double ba = (double)Fmt<DTA>::BB / Fmt<DTA>::BW, bb = (double)Fmt<DTB>::BB / Fmt<DTB>::BW;
    long ra = 0, rb = 0;
    for (int i = 0; i < na; ++i) ra += sa[i].rows;
    for (int i = 0; i < nb; ++i) rb += sb[i].rows;
    if (ra <= 0 || rb <= 0) return NTK_E_SHAPE;
    const int total_wg = max_workgroups();
    int wa = (int)(total_wg * (ra * ba) / (ra * ba + rb * bb) + 0.5);
    wa = std::min(std::max(wa, 1), total_wg - 1);
    GemvLaunch A, B;
    int rc = prepare_quant<DTA>(sa, na, x, in, norm_w, eps, nullptr, 0, wa, A);
    if (rc == NTK_OK) rc = prepare_quant<DTB>(sb, nb, x, in, norm_w, eps, nullptr, 0, total_wg - wa, B);
    if (rc != NTK_OK) return rc;
    // the pair kernel is the aligned fast form of both formats: anything else goes out as two launches (NTK_E_ALIGN -> caller)
    if (!A.xfast || !B.xfast || A.nwaves != B.nwaves || A.a16 != A16_OK<DTA> || B.a16 != A16_OK<DTB>) return NTK_E_ALIGN;
    for (int i = 0; i < na; ++i) if (A.p.seg[i].delta != 0 && A16_OK<DTA>) return NTK_E_ALIGN;
    using PairFn = void (*)(const GemvParams, const GemvParams, int);
    const size_t lds = std::max(A.lds, B.lds);
    static const PairFn table[2] = {gemv_quant_pair_kernel<DTA, DTB, false>, gemv_quant_pair_kernel<DTA, DTB, true>};
    if (lds > 64 * 1024) {
        static bool once = hipFuncSetAttribute((const void*)table[0], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess &&
                           hipFuncSetAttribute((const void*)table[1], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) == hipSuccess;
        if (!once || lds > 160 * 1024) return NTK_E_SHAPE;
    }
    hipLaunchKernelGGL(table[norm_w ? 1 : 0], dim3(A.grid + B.grid), dim3(64 * A.nwaves), lds, st, A.p, B.p, A.grid);
    return last_launch_status();
}

static int dispatch_quant(int dt, const ntk_gemv_seg* segs, int nseg, const float* x, int in, const float* norm_w,
                          float eps, const float* resid, int silu_pair, hipStream_t st, int xi_mode = XI_DEFAULT) {
    switch (dt) {
        case NTK_DT_Q8_0: return launch_quant<NTK_DT_Q8_0>(segs, nseg, x, in, norm_w, eps, resid, silu_pair, st);
        case NTK_DT_Q4_0: return launch_quant<NTK_DT_Q4_0>(segs, nseg, x, in, norm_w, eps, resid, silu_pair, st);
        case NTK_DT_Q4_K: return launch_quant<NTK_DT_Q4_K>(segs, nseg, x, in, norm_w, eps, resid, silu_pair, st, xi_mode);
        case NTK_DT_Q5_K: return launch_quant<NTK_DT_Q5_K>(segs, nseg, x, in, norm_w, eps, resid, silu_pair, st);
        case NTK_DT_Q6_K: return launch_quant<NTK_DT_Q6_K>(segs, nseg, x, in, norm_w, eps, resid, silu_pair, st, xi_mode);
        default: return NTK_E_DTYPE;
    }
}

template <bool ADD>
static int launch_dense(float* y, const void* W, const float* x, int out, int in, int dt, hipStream_t st) {
    if (out == 0) return NTK_OK;
    const int grid = std::min((out + 3) / 4, 2048);
    if (dt == NTK_DT_F32)
        hipLaunchKernelGGL((gemv_dense_kernel<float, ADD>), dim3(grid), dim3(256), 0, st, y, (const float*)W, x, out, in);
    else if (dt == NTK_DT_BF16)
        hipLaunchKernelGGL((gemv_dense_kernel<uint16_t, ADD, true>), dim3(grid), dim3(256), 0, st, y, (const uint16_t*)W, x, out, in);
    else
        hipLaunchKernelGGL((gemv_dense_kernel<uint16_t, ADD>), dim3(grid), dim3(256), 0, st, y, (const uint16_t*)W, x, out, in);
    return last_launch_status();
}

}  // namespace ntk

extern "C" {

#ifdef NTK_GEMV_TRACE
NTK_EXTRA_API int ntk_debug_gemv_trace(unsigned long long* out, size_t n) {   // n <= GT_SLOTS * GT_WG * GT_EV
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(ntk::g_gemv_trace), n * sizeof(unsigned long long)) == hipSuccess ? 0 : -3;
}
#endif

int ntk_decode_arena_acquire(void) {
    ntk::ArenaDev* a = ntk::arena_dev(true);
    int free_ = 0;
    return a && a->owned.compare_exchange_strong(free_, 1) ? (int)(a - ntk::g_arena_dev) : -1;
}
void ntk_decode_arena_release(int device) {   // by index: whichever device is current when the owner closes
    if (device >= 0 && device < ntk::kArenaDevices) ntk::g_arena_dev[device].owned.store(0);
}
float* ntk_decode_arena_slot(int slot) {
    const ntk::ArenaDev* a = ntk::arena_dev(true);
    return a && slot >= NTK_ARENA_HIDDEN && slot <= NTK_ARENA_GATE ? const_cast<float*>(a->addr[slot]) : nullptr;
}
int ntk_debug_gemv_static_x(void) { return ntk::t_last_static_x; }

size_t ntk_q8l_bytes(int rows, int in_features) { return ntk::q8l_bytes(rows, in_features); }
int ntk_q8l_pack(void* dst, const void* raw, int rows, int in_features, void* stream) {
    if (!dst || !raw) return NTK_E_NULL;
    return ntk::q8l_pack(dst, raw, rows, in_features, false, ntk::resolve_stream(stream));
}
int ntk_q8l_unpack(void* raw, const void* packed, int rows, int in_features, void* stream) {
    if (!raw || !packed) return NTK_E_NULL;
    return ntk::q8l_pack(raw, packed, rows, in_features, true, ntk::resolve_stream(stream));
}

int ntk_gemv(float* y, const void* W, const float* x, int out_features, int in_features, int weight_dtype, void* stream) {
    if (!y || !W || !x) return NTK_E_NULL;
    if (out_features < 0 || in_features <= 0) return NTK_E_SHAPE;
    hipStream_t st = ntk::resolve_stream(stream);
    if (weight_dtype == NTK_DT_F32 || weight_dtype == NTK_DT_F16 || weight_dtype == NTK_DT_BF16)
        return ntk::launch_dense<false>(y, W, x, out_features, in_features, weight_dtype, st);
    if (!ntk::is_quant(weight_dtype)) return NTK_E_DTYPE;
    ntk_gemv_seg seg{W, y, out_features, weight_dtype};
    return ntk::dispatch_quant(weight_dtype, &seg, 1, x, in_features, nullptr, 0.0f, nullptr, 0, st);
}

int ntk_gemv_add(float* y, const void* W, const float* x, int out_features, int in_features, int weight_dtype, void* stream) {
    if (!y || !W || !x) return NTK_E_NULL;
    if (out_features < 0 || in_features <= 0) return NTK_E_SHAPE;
    if (weight_dtype != NTK_DT_F16) return NTK_E_DTYPE;   // reference gemm.cu:861-869
    return ntk::launch_dense<true>(y, W, x, out_features, in_features, weight_dtype, ntk::resolve_stream(stream));
}


static int gemv_fused_form(const ntk_gemv_seg* segs, int nseg, const float* x, int in_features, const float* norm_w, float eps,
                           const float* resid, int silu_pair, void* stream, int xi_mode) {
    if (!segs || !x) return NTK_E_NULL;
    if (nseg < 1 || nseg > ntk::MAX_SEG) return NTK_E_SHAPE;
    if (segs[0].dtype == NTK_DT_F16 || segs[0].dtype == NTK_DT_BF16) {   // unquantised 16-bit rows: gemv_dense16.hip, segments of one dtype
        for (int i = 1; i < nseg; ++i)
            if (segs[i].dtype != segs[0].dtype) return NTK_E_DTYPE;
        return ntk::dense16_gemv_fused(segs, nseg, x, in_features, norm_w, eps, resid, silu_pair, ntk::resolve_stream(stream));
    }
    ntk_gemv_seg a[3], b[3];
    int na = 0, nb = 0;
    for (int i = 0; i < nseg; ++i) {
        if (!ntk::is_quant(segs[i].dtype)) return NTK_E_DTYPE;
        if (segs[i].dtype == segs[0].dtype) a[na++] = segs[i];
        else if (nb == 0 || segs[i].dtype == b[0].dtype) b[nb++] = segs[i];
        else return NTK_E_DTYPE;   // three formats in one call
    }
    hipStream_t st = ntk::resolve_stream(stream);
    if (nb == 0) return ntk::dispatch_quant(segs[0].dtype, segs, nseg, x, in_features, norm_w, eps, resid, silu_pair, st, xi_mode);
    // two formats: supported as one launch for the K-quant mixes of llama.cpp's Q4_K_M, plain projections only
    if (resid || silu_pair) return NTK_E_DTYPE;
    const int da = a[0].dtype, db = b[0].dtype;
    if (da == NTK_DT_Q4_K && db == NTK_DT_Q6_K) return ntk::launch_pair<NTK_DT_Q4_K, NTK_DT_Q6_K>(a, na, b, nb, x, in_features, norm_w, eps, st);
    if (da == NTK_DT_Q6_K && db == NTK_DT_Q4_K) return ntk::launch_pair<NTK_DT_Q4_K, NTK_DT_Q6_K>(b, nb, a, na, x, in_features, norm_w, eps, st);
    if (da == NTK_DT_Q4_K && db == NTK_DT_Q5_K) return ntk::launch_pair<NTK_DT_Q4_K, NTK_DT_Q5_K>(a, na, b, nb, x, in_features, norm_w, eps, st);
    if (da == NTK_DT_Q5_K && db == NTK_DT_Q4_K) return ntk::launch_pair<NTK_DT_Q4_K, NTK_DT_Q5_K>(b, nb, a, na, x, in_features, norm_w, eps, st);
    return NTK_E_DTYPE;
}

int ntk_gemv_fused(const ntk_gemv_seg* segs, int nseg, const float* x, int in_features, const float* norm_w, float eps,
                   const float* resid, int silu_pair, void* stream) {
    return gemv_fused_form(segs, nseg, x, in_features, norm_w, eps, resid, silu_pair, stream, ntk::XI_DEFAULT);
}
// parity instrumentation: ntk_gemv_fused with the activation form of the Q4_K / Q6_K launches chosen by the CALL (1: the integer-activation
// decoders whenever the launch is eligible, 0: never, -1: the library's size rule) -- so that the tests reach both decoders at small sizes
int ntk_debug_gemv_fused_form(const ntk_gemv_seg* segs, int nseg, const float* x, int in_features, const float* norm_w, float eps,
                              const float* resid, int silu_pair, int integer_activations, void* stream) {
    if (integer_activations < -1 || integer_activations > 1) return NTK_E_SHAPE;
    return gemv_fused_form(segs, nseg, x, in_features, norm_w, eps, resid, silu_pair, stream, integer_activations);
}

}  // extern "C"
