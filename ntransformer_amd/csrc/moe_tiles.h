// moe_tiles.h -- how the grouped expert GEMM (moe_gemm.hip) cuts the expert-major work list into tiles, stated once in plain C++ so that a host program can
// check it (tests/moe_tiles_check.cpp) and the kernel's parallel form can be read against it.
//
// The list: offsets[E + 1] and pairs[n_pairs], expert e owning entries [offsets[e], offsets[e + 1]).  A TILE is up to MOE_TILE consecutive entries of ONE
// expert's range; expert e has ceil(count_e / MOE_TILE) tiles, and the tiles are numbered expert by expert.  Over a list that is a partition of
// [0, n_pairs):   sum_e ceil(c_e / 16) <= sum_e c_e / 16 + #(experts with c_e > 0)  <=  ceil(n_pairs / 16) + E   = moe_tile_bound: the grid.
// Ranges are read through the clamp of moe.hip's moe_expert_range (begin >= 0, end <= n_pairs), so a table that is not ours names entries inside the list
// or nothing; tiles beyond the bound are then simply not run.
#pragma once

#ifdef __HIPCC__
#define MOE_TILES_FN __host__ __device__ inline
#else
#define MOE_TILES_FN inline
#endif

constexpr int MOE_TILE = 16;   // entries per tile = the MFMA's N

MOE_TILES_FN int moe_tile_bound(int n_pairs, int E) { return (n_pairs + MOE_TILE - 1) / MOE_TILE + E; }

// the clamped range of expert e and its number of tiles
MOE_TILES_FN int moe_range_tiles(const int* offsets, int e, int n_pairs, int& beg, int& end) {
    beg = offsets[e]; end = offsets[e + 1];
    if (beg < 0) beg = 0;
    if (end > n_pairs) end = n_pairs;
    return end > beg ? (end - beg + MOE_TILE - 1) / MOE_TILE : 0;
}

// tile number `tile` -> its expert, its first entry and the end of the expert's range (the tile is [first, min(first + MOE_TILE, end)));
// false: there are fewer tiles.  The kernel computes the same thing with one thread per expert and a prefix sum.
MOE_TILES_FN bool moe_tile_find(const int* offsets, int E, int n_pairs, int tile, int& expert, int& first, int& end) {
    int start = 0;
    for (int e = 0; e < E; ++e) {
        int beg, en;
        const int n = moe_range_tiles(offsets, e, n_pairs, beg, en);
        if (tile >= start && tile < start + n) { expert = e; first = beg + MOE_TILE * (tile - start); end = en; return true; }
        start += n;
    }
    return false;
}
