// moe_row.hip -- the ROW form of the routed expert FFN: one row (T = 1, the decode token and every other one-row pass), the bits of moe.hip's three launches.
// At one row pair k is simply expert ids[k]: there is no work list, nothing walks E offsets, and no product crosses global memory.  Three launches:
//
//   moe_row_logits_kernel    one WAVE per expert (grid ceil(E / 4)): the E router dots side by side, moe_router_dot's chain, logits to the workspace.
//   moe_row_gate_up_kernel   grid (ceil(inter / R), K).  Every workgroup stages xn into LDS once (its waves then read it in 16-byte LDS reads) while wave 0
//                            redoes the selection from the E logits (moe_select, moe_softmax_store: the T-row kernel's code); its expert is ids[blockIdx.y].
//                            Workgroup (0, 0) leaves ids and w in the workspace.  A wave takes rows wave, wave + 4, ... of the block: the NEXT gate and up rows
//                            are fetched into registers (16-byte global loads) before this row's two chains run and are committed to the wave's LDS images
//                            after them.  The images are wave-private: no workgroup barrier in the row loop.
//   moe_row_down_kernel      grid ceil(hidden / R).  The K act rows are staged into LDS (K inter floats); the K x R (expert, row) tasks go round the waves with
//                            the same fetch-ahead; products land in an LDS part[k][r]; one barrier; thread r sums its row over k ascending with the T-row
//                            kernel's fmaf chain and adds resid.  No global part, no fence.
//
// The arithmetic is moe_core.hip.h's, shared with moe.hip: one wave per weight row, lane l the 32-column units l, l + 64, ..., one fmaf chain in ascending
// column order, wave_sum -- a row is never packed with another, whatever its length.  Reading x from LDS instead of L2 changes no value.
#include <algorithm>
#include "moe_core.hip.h"

namespace ntk {

constexpr int kRowWaves = 4;             // waves per workgroup
constexpr int kRowMaxR = 16;             // most output rows a down workgroup owns
constexpr size_t kRowLdsMax = NTK_MOE_ROW_LDS_MAX;   // dynamic LDS a launch may ask for: gfx950's 160 KiB less the kernels' static arrays

struct MoeRowArgs {
    const float* xn; const float* router; float* logits;
    const uint8_t* wg; const uint8_t* wu; const uint8_t* wd;
    const float* resid; float* y; float* act; int* ids; float* w;
    int dt_g, dt_u, dt_d;
    unsigned rb_g, rb_u, rb_d, img_g, img_u, img_d;   // row bytes and LDS image bytes
    int hidden, inter, E, K, vec, rows_gu, rows_d;
};

// ---- a row on its way from global memory to the wave's image: fetch (into registers, nothing waits) and commit (registers to LDS).  moe_stage_row's
//      geometry: 2-byte pieces up to the first 16-byte boundary, 16-byte pieces (piece i in lane i % 64, register i / 64), 2-byte pieces behind the last.
//      NB = 0: rows longer than 64 NB pieces -- nothing is fetched ahead and commit is moe_stage_row. ----
template <int NB> struct MoeRowRegs {
    moe_u32x4 body[NB ? NB : 1];
    uint16_t head, tail;
};

template <int NB>
__device__ __forceinline__ void moe_row_fetch(MoeRowRegs<NB>& r, const uint8_t* g, unsigned rb, int lane) {
    if constexpr (NB > 0) {
        const unsigned shift = (unsigned)((uintptr_t)g & 15u);
        unsigned head = (16u - shift) & 15u;
        if (head > rb) head = rb;
        const unsigned body = (rb - head) / 16u, tail = rb - head - 16u * body, t0 = head + 16u * body;
        r.head = (unsigned)lane < head / 2u ? reinterpret_cast<const uint16_t*>(g)[lane] : (uint16_t)0;
        const moe_u32x4* src = reinterpret_cast<const moe_u32x4*>(g + head);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const unsigned i = (unsigned)lane + 64u * j;
            if (i < body) r.body[j] = src[i];
        }
        r.tail = (unsigned)lane < tail / 2u ? reinterpret_cast<const uint16_t*>(g + t0)[lane] : (uint16_t)0;
    }
}

template <int NB>
__device__ __forceinline__ int moe_row_commit(const MoeRowRegs<NB>& r, uint8_t* st, const uint8_t* g, unsigned rb, int lane) {
    if constexpr (NB == 0) {
        return moe_stage_row(st, g, rb, lane);
    } else {
        const unsigned shift = (unsigned)((uintptr_t)g & 15u);
        unsigned head = (16u - shift) & 15u;
        if (head > rb) head = rb;
        const unsigned body = (rb - head) / 16u, tail = rb - head - 16u * body, t0 = head + 16u * body;
        if ((unsigned)lane < head / 2u) reinterpret_cast<uint16_t*>(st + shift)[lane] = r.head;
        moe_u32x4* dst = reinterpret_cast<moe_u32x4*>(st + shift + head);
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const unsigned i = (unsigned)lane + 64u * j;
            if (i < body) dst[i] = r.body[j];
        }
        if ((unsigned)lane < tail / 2u) reinterpret_cast<uint16_t*>(st + shift + t0)[lane] = r.tail;
        return (int)shift;
    }
}

// the image is written and read by different lanes of ONE wave: LDS serves a wave's accesses in order, the compiler must keep them in order too
__device__ __forceinline__ void moe_row_image_fence() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- logits: grid ceil(E / 4), 256 threads, one wave per expert ----
__global__ __launch_bounds__(64 * kRowWaves) void moe_row_logits_kernel(const MoeRowArgs a) {
    const int lane = threadIdx.x & 63, e = (int)blockIdx.x * kRowWaves + (int)(threadIdx.x >> 6);
    if (e >= a.E) return;
    const float s = moe_router_dot(a.xn, a.router + (size_t)e * a.hidden, a.hidden, a.vec, lane);
    if (lane == 0) a.logits[e] = s;
}

// ---- gate | up: grid (ceil(inter / rows_gu), K), 256 threads; dynamic LDS: xn [hidden] | per wave: gate image, up image ----
template <int NB>
__global__ __launch_bounds__(64 * kRowWaves) void moe_row_gate_up_kernel(const MoeRowArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t moe_row_lds[];
    __shared__ int s_ids[kMoeMaxK];
    __shared__ float s_w[kMoeMaxK];
    float* const s_x = reinterpret_cast<float*>(moe_row_lds);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int i = threadIdx.x; i < a.hidden / 4; i += 64 * kRowWaves) reinterpret_cast<float4*>(s_x)[i] = reinterpret_cast<const float4*>(a.xn)[i];
    if (wave == 0) {
        float sel[kMoeMaxK];
        int sel_id[kMoeMaxK];
        moe_select(a.logits, a.E, a.K, lane, sel, sel_id);
        if (lane == 0) moe_softmax_store(sel, sel_id, a.K, s_ids, s_w);
    }
    __syncthreads();
    const int k = blockIdx.y;
    if (blockIdx.x == 0 && k == 0 && (int)threadIdx.x < a.K) {
        a.ids[threadIdx.x] = s_ids[threadIdx.x];
        a.w[threadIdx.x] = s_w[threadIdx.x];
    }
    int e = __builtin_amdgcn_readfirstlane(s_ids[k]);
    e = e < 0 ? 0 : e >= a.E ? a.E - 1 : e;   // (before any address is formed)
    uint8_t* const st_g = moe_row_lds + (size_t)a.hidden * 4 + (size_t)wave * (a.img_g + a.img_u);
    uint8_t* const st_u = st_g + a.img_g;
    const int n_units = a.hidden / 32, row0 = blockIdx.x * a.rows_gu;
    const int row_end = row0 + a.rows_gu < a.inter ? row0 + a.rows_gu : a.inter;
    const uint8_t* const base_g = a.wg + (size_t)e * (size_t)a.inter * a.rb_g;
    const uint8_t* const base_u = a.wu + (size_t)e * (size_t)a.inter * a.rb_u;
    const float* const x[1] = {s_x};
    MoeRowRegs<NB> rg, ru;
    int row = row0 + wave;
    if (row < row_end) {
        moe_row_fetch<NB>(rg, base_g + (size_t)row * a.rb_g, a.rb_g, lane);
        moe_row_fetch<NB>(ru, base_u + (size_t)row * a.rb_u, a.rb_u, lane);
    }
    for (; row < row_end; row += kRowWaves) {
        moe_row_image_fence();   // (the previous row's reads are behind us)
        const int og = moe_row_commit<NB>(rg, st_g, base_g + (size_t)row * a.rb_g, a.rb_g, lane);
        const int ou = moe_row_commit<NB>(ru, st_u, base_u + (size_t)row * a.rb_u, a.rb_u, lane);
        moe_row_image_fence();
        if (row + kRowWaves < row_end) {   // the next rows' loads fly while this row's chains run
            moe_row_fetch<NB>(rg, base_g + (size_t)(row + kRowWaves) * a.rb_g, a.rb_g, lane);
            moe_row_fetch<NB>(ru, base_u + (size_t)(row + kRowWaves) * a.rb_u, a.rb_u, lane);
        }
        float g[1], u[1];
        moe_row_dots<1>(g, a.dt_g, st_g, og, n_units, lane, x);
        moe_row_dots<1>(u, a.dt_u, st_u, ou, n_units, lane, x);
        if (lane == 0) a.act[(size_t)k * a.inter + row] = moe_silu_mul(g[0], u[0]);
    }
}

// ---- down: grid ceil(hidden / rows_d), 256 threads; dynamic LDS: act [K][inter] | per wave: one image ----
template <int NB>
__global__ __launch_bounds__(64 * kRowWaves) void moe_row_down_kernel(const MoeRowArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t moe_row_lds[];
    __shared__ int s_ids[kMoeMaxK];
    __shared__ float s_w[kMoeMaxK];
    __shared__ float s_part[kMoeMaxK * kRowMaxR];
    float* const s_act = reinterpret_cast<float*>(moe_row_lds);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    for (int i = threadIdx.x; i < a.K * (a.inter / 4); i += 64 * kRowWaves) reinterpret_cast<float4*>(s_act)[i] = reinterpret_cast<const float4*>(a.act)[i];
    if ((int)threadIdx.x < a.K) {   // what the gate | up launch's workgroup (0, 0) left
        const int e = a.ids[threadIdx.x];
        s_ids[threadIdx.x] = e < 0 ? 0 : e >= a.E ? a.E - 1 : e;
        s_w[threadIdx.x] = a.w[threadIdx.x];
    }
    __syncthreads();
    uint8_t* const st = moe_row_lds + (size_t)a.K * a.inter * 4 + (size_t)wave * a.img_d;
    const int n_units = a.inter / 32, row0 = blockIdx.x * a.rows_d;
    const int nr = a.hidden - row0 < a.rows_d ? a.hidden - row0 : a.rows_d, n_tasks = a.K * nr;
    // task i: pair k = i / nr, output row row0 + i % nr (neighbouring waves: neighbouring rows of one expert)
    auto row_of = [&](int i) { return a.wd + ((size_t)s_ids[i / nr] * (size_t)a.hidden + (size_t)(row0 + i % nr)) * a.rb_d; };
    MoeRowRegs<NB> rr;
    int i = wave;
    if (i < n_tasks) moe_row_fetch<NB>(rr, row_of(i), a.rb_d, lane);
    for (; i < n_tasks; i += kRowWaves) {
        moe_row_image_fence();
        const int o = moe_row_commit<NB>(rr, st, row_of(i), a.rb_d, lane);
        moe_row_image_fence();
        if (i + kRowWaves < n_tasks) moe_row_fetch<NB>(rr, row_of(i + kRowWaves), a.rb_d, lane);
        const int k = i / nr;
        const float* const x[1] = {s_act + (size_t)k * a.inter};
        float d[1];
        moe_row_dots<1>(d, a.dt_d, st, o, n_units, lane, x);
        if (lane == 0) s_part[k * kRowMaxR + i % nr] = d[0];
    }
    __syncthreads();
    if ((int)threadIdx.x < nr) {   // resid + the K products in ascending k
        const int r = threadIdx.x;
        float s = 0.0f;
        for (int k = 0; k < a.K; ++k) s = fmaf(s_w[k], s_part[k * kRowMaxR + r], s);
        a.y[row0 + r] = a.resid[row0 + r] + s;
    }
}

// 16-byte pieces per lane a row of rb bytes needs in flight -> the instantiation that holds them (0: none does, rows are staged without fetch-ahead)
static int moe_row_nb(unsigned rb) {
    const unsigned per_lane = (rb / 16u + 63u) / 64u;
    return per_lane <= 4 ? 4 : per_lane <= 12 ? 12 : 0;
}

// rows per workgroup: the most of 8, 4, 2, 1 per wave that still leaves min_wgs workgroups (the device has 256 CUs)
static int moe_row_block(int rows, int groups, int most_per_wave, int min_wgs) {
    for (int per_wave = most_per_wave; per_wave > 1; per_wave /= 2) {
        const int r = per_wave * kRowWaves;
        if ((long long)((rows + r - 1) / r) * groups >= min_wgs) return r;
    }
    return kRowWaves;
}

struct MoeRowPlan { size_t lds_gu, lds_d; unsigned rb_g, rb_u, rb_d; };
static bool moe_row_plan(int dt_g, int dt_u, int dt_d, int hidden, int inter, int K, MoeRowPlan& p) {
    if (!moe_type_ok(dt_g) || !moe_type_ok(dt_u) || !moe_type_ok(dt_d) || hidden <= 0 || inter <= 0 || K < 1 || K > kMoeMaxK) return false;
    const size_t rg = ntk_row_bytes(dt_g, hidden), ru = ntk_row_bytes(dt_u, hidden), rd = ntk_row_bytes(dt_d, inter);
    if (!rg || !ru || !rd || rg > 0x7FFFFFFFu || ru > 0x7FFFFFFFu || rd > 0x7FFFFFFFu) return false;
    p.rb_g = (unsigned)rg; p.rb_u = (unsigned)ru; p.rb_d = (unsigned)rd;
    p.lds_gu = (size_t)hidden * 4 + (size_t)kRowWaves * ((size_t)moe_image_bytes(p.rb_g) + moe_image_bytes(p.rb_u));
    p.lds_d = (size_t)K * inter * 4 + (size_t)kRowWaves * moe_image_bytes(p.rb_d);
    return true;
}

template <typename Fn> static bool moe_row_lds_attr(Fn fn) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRowLdsMax) == hipSuccess;   // (beside the static arrays)
}

}  // namespace ntk

extern "C" size_t ntk_moe_row_lds_bytes(int dt_gate, int dt_up, int dt_down, int hidden, int inter, int K) {
    ntk::MoeRowPlan p;
    if (!ntk::moe_row_plan(dt_gate, dt_up, dt_down, hidden, inter, K, p)) return 0;
    return p.lds_gu > p.lds_d ? p.lds_gu : p.lds_d;
}

extern "C" int ntk_moe_ffn_row(float* y, const float* resid, const float* xn, const float* router, const void* w_gate, int dt_gate, const void* w_up, int dt_up,
                               const void* w_down, int dt_down, int hidden, int inter, int E, int K, void* ws, size_t ws_bytes, void* stream) {
    using namespace ntk;
    if (!y || !resid || !xn || !router || !w_gate || !w_up || !w_down || !ws) return NTK_E_NULL;
    if (!moe_type_ok(dt_gate) || !moe_type_ok(dt_up) || !moe_type_ok(dt_down)) return NTK_E_DTYPE;
    if (E < 1 || E > kMoeMaxE || K < 1 || K > kMoeMaxK || K > E || hidden <= 0 || inter <= 0) return NTK_E_SHAPE;
    MoeRowPlan p;
    if (!moe_row_plan(dt_gate, dt_up, dt_down, hidden, inter, K, p)) return NTK_E_SHAPE;   // columns that are not whole blocks
    if (p.lds_gu > kRowLdsMax || p.lds_d > kRowLdsMax) return NTK_E_SHAPE;                 // (ntk_moe_row_lds_bytes beyond NTK_MOE_ROW_LDS_MAX)
    size_t off[NTK_MOE_WS_SECTIONS];
    const size_t need = ntk_moe_workspace_layout(1, E, K, inter, hidden, off);
    if (need == 0 || ws_bytes < need || (size_t)K * hidden < (size_t)E) return NTK_E_SHAPE;   // (the logits live in the part section: K hidden floats)
    if (((uintptr_t)y | (uintptr_t)resid | (uintptr_t)xn | (uintptr_t)ws) % 16 != 0 || ((uintptr_t)w_gate | (uintptr_t)w_up | (uintptr_t)w_down) % 2 != 0)
        return NTK_E_ALIGN;
    uint8_t* const base = static_cast<uint8_t*>(ws);
    MoeRowArgs a{};
    a.xn = xn; a.router = router; a.logits = reinterpret_cast<float*>(base + off[NTK_MOE_WS_PART]);
    a.wg = (const uint8_t*)w_gate; a.wu = (const uint8_t*)w_up; a.wd = (const uint8_t*)w_down;
    a.resid = resid; a.y = y; a.act = reinterpret_cast<float*>(base + off[NTK_MOE_WS_ACT]);
    a.ids = reinterpret_cast<int*>(base + off[NTK_MOE_WS_IDS]); a.w = reinterpret_cast<float*>(base + off[NTK_MOE_WS_W]);
    a.dt_g = dt_gate; a.dt_u = dt_up; a.dt_d = dt_down;
    a.rb_g = p.rb_g; a.rb_u = p.rb_u; a.rb_d = p.rb_d;
    a.img_g = moe_image_bytes(p.rb_g); a.img_u = moe_image_bytes(p.rb_u); a.img_d = moe_image_bytes(p.rb_d);
    a.hidden = hidden; a.inter = inter; a.E = E; a.K = K;
    a.vec = hidden % 4 == 0 && ((uintptr_t)xn | (uintptr_t)router) % 16 == 0 ? 1 : 0;   // (ntk_moe_route's rule: the same chain)
    a.rows_gu = moe_row_block(inter, K, 8, 512);
    // (every down workgroup stages the K act rows: where those are large, fewer workgroups with more rows each)
    a.rows_d = moe_row_block(hidden, 1, kRowMaxR / kRowWaves, p.lds_d <= 48 * 1024 ? 512 : 256);
    static const bool attr = moe_row_lds_attr(moe_row_gate_up_kernel<0>) && moe_row_lds_attr(moe_row_gate_up_kernel<4>) && moe_row_lds_attr(moe_row_gate_up_kernel<12>) &&
                             moe_row_lds_attr(moe_row_down_kernel<0>) && moe_row_lds_attr(moe_row_down_kernel<4>) && moe_row_lds_attr(moe_row_down_kernel<12>);
    if (!attr) return NTK_E_LAUNCH;
    hipStream_t st = resolve_stream(stream);
    const dim3 threads(64 * kRowWaves);
    hipLaunchKernelGGL(moe_row_logits_kernel, dim3((unsigned)((E + kRowWaves - 1) / kRowWaves)), threads, 0, st, a);
    const dim3 grid_gu((unsigned)((inter + a.rows_gu - 1) / a.rows_gu), (unsigned)K);
    const int nb_gu = std::min(moe_row_nb(p.rb_g), moe_row_nb(p.rb_u));   // (0 where either row is too long to fetch ahead)
    const int nb_pair = nb_gu == 0 ? 0 : std::max(moe_row_nb(p.rb_g), moe_row_nb(p.rb_u));
    if (nb_pair == 4) hipLaunchKernelGGL(moe_row_gate_up_kernel<4>, grid_gu, threads, p.lds_gu, st, a);
    else if (nb_pair == 12) hipLaunchKernelGGL(moe_row_gate_up_kernel<12>, grid_gu, threads, p.lds_gu, st, a);
    else hipLaunchKernelGGL(moe_row_gate_up_kernel<0>, grid_gu, threads, p.lds_gu, st, a);
    const dim3 grid_d((unsigned)((hidden + a.rows_d - 1) / a.rows_d));
    const int nb_d = moe_row_nb(p.rb_d);
    if (nb_d == 4) hipLaunchKernelGGL(moe_row_down_kernel<4>, grid_d, threads, p.lds_d, st, a);
    else if (nb_d == 12) hipLaunchKernelGGL(moe_row_down_kernel<12>, grid_d, threads, p.lds_d, st, a);
    else hipLaunchKernelGGL(moe_row_down_kernel<0>, grid_d, threads, p.lds_d, st, a);
    return last_launch_status();
}
