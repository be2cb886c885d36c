// tests/moe_tiles_check.cpp -- csrc/moe_tiles.h on the host, nothing but that header (tests/test_moe_gemm_cpu.py builds and runs it).
// Reads cases from stdin, one per line:  E n_pairs off_0 ... off_E   and prints for each   "case <tiles> <bound>"  followed by one line per tile
// "tile <number> <expert> <first> <end_of_tile>"; the tiles are enumerated by asking moe_tile_find for 0, 1, ... up to 4 x the bound (a table that is
// not a partition may have more tiles than the bound; the kernel's grid stops at the bound).
#include <cstdio>
#include <vector>

#include "../ntransformer_amd/csrc/moe_tiles.h"

int main() {
    int E, n_pairs;
    while (std::scanf("%d %d", &E, &n_pairs) == 2) {
        std::vector<int> off(E + 1);
        for (int i = 0; i <= E; ++i)
            if (std::scanf("%d", &off[i]) != 1) return 2;
        const int bound = moe_tile_bound(n_pairs, E);
        std::vector<int> lines;
        int tiles = 0;
        for (int t = 0; t < 4 * bound + 4; ++t) {
            int e = -1, first = -1, end = -1;
            if (!moe_tile_find(off.data(), E, n_pairs, t, e, first, end)) break;
            ++tiles;
            lines.push_back(t); lines.push_back(e); lines.push_back(first); lines.push_back(first + MOE_TILE < end ? first + MOE_TILE : end);
        }
        std::printf("case %d %d\n", tiles, bound);
        for (size_t i = 0; i < lines.size(); i += 4) std::printf("tile %d %d %d %d\n", lines[i], lines[i + 1], lines[i + 2], lines[i + 3]);
    }
    return 0;
}
