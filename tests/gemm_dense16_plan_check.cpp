// tests/gemm_dense16_plan_check.cpp -- host program of tests/test_gemm_dense16_cpu.py: nothing but csrc/gemm_dense16_plan.h.  One argument per call,
// "dtypes:T:in:rows:misaligned" (dtypes, rows: comma separated, one per matrix; misaligned: index of the call's pointer that is off the 16-byte grid -- W_i
// and Y_i of every matrix, then X, resid, workspace -- or -1), one line per argument: the refusal, or the plan and what walking its grid finds -- how
// often each (row, token) of the call is written, and the last workspace byte the launch addresses.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include "../ntransformer_amd/csrc/gemm_dense16_plan.h"

using namespace ntk;

static std::vector<int> ints(const std::string& s) {
    std::vector<int> v;
    size_t at = 0;
    while (at <= s.size()) {
        const size_t c = s.find(',', at);
        v.push_back(atoi(s.substr(at, c == std::string::npos ? std::string::npos : c - at).c_str()));
        if (c == std::string::npos) break;
        at = c + 1;
    }
    return v;
}

int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        std::vector<std::string> f;
        std::string s = argv[a];
        size_t at = 0;
        for (;;) {
            const size_t c = s.find(':', at);
            f.push_back(s.substr(at, c == std::string::npos ? std::string::npos : c - at));
            if (c == std::string::npos) break;
            at = c + 1;
        }
        if (f.size() != 5) { fprintf(stderr, "bad argument %s\n", argv[a]); return 2; }
        const std::vector<int> dtypes = ints(f[0]), rows = ints(f[3]);
        const int T = atoi(f[1].c_str()), in = atoi(f[2].c_str()), bad = atoi(f[4].c_str()), nseg = (int)rows.size();
        if (dtypes.size() != rows.size()) { fprintf(stderr, "bad argument %s\n", argv[a]); return 2; }
        std::vector<uintptr_t> ptrs;
        for (int i = 0; i < 2 * nseg + 3; ++i) ptrs.push_back((uintptr_t)0x10000 * (i + 1) + (i == bad ? 4 : 0));
        const Dense16Plan p = gemm_dense16_plan(rows.data(), dtypes.data(), nseg, T, in, ptrs.data(), (int)ptrs.size());
        printf("%s : status=%d", argv[a], p.status);
        if (p.status != NTK_OK) { printf("\n"); continue; }
        // walk the grid as the kernel does: workgroup -> (row tile, chunk) -> matrix -> the wave's tiles of 16 rows x the chunk's token blocks
        std::vector<std::vector<unsigned char>> seen(nseg);
        for (int i = 0; i < nseg; ++i) seen[i].assign((size_t)(rows[i] / 16) * T, 0);
        int worst = 0;
        bool inside = true;
        for (unsigned b = 0; b < p.grid_x; ++b) {
            int tile, chunk;
            if (!gd_map(b, p.tiles, p.chunks, tile, chunk)) continue;
            int sg = 0;
            if (nseg > 1 && tile >= p.seg[1].tile0) sg = 1;
            if (nseg > 2 && tile >= p.seg[2].tile0) sg = 2;
            if (tile - p.seg[sg].tile0 >= p.seg[sg].tiles || chunk >= p.chunks) inside = false;
            for (int w = 0; w < GD_WAVES; ++w)
                for (int r = 0; r < p.rt; ++r) {
                    const int row = (tile - p.seg[sg].tile0) * 64 * p.rt + w * 16 * p.rt + 16 * r;
                    if (row >= rows[sg]) continue;
                    for (int tb = 0; tb < p.ntb; ++tb)
                        for (int j = 0; j < 16; ++j) {
                            const int t = chunk * GD_TOK + tb * 16 + j;
                            if (t >= T) continue;
                            unsigned char& n = seen[sg][(size_t)(row / 16) * T + t];
                            if (n < 255) ++n;
                        }
                }
        }
        int least = 255;
        for (int i = 0; i < nseg; ++i)
            for (unsigned char n : seen[i]) { if (n > worst) worst = n; if (n < least) least = n; }
        // the last workspace byte addressed: the last piece of the last step's record of the last chunk (read by the kernel, written by the BF16 pre-pass),
        // F16: the last token's 1 / s
        size_t need = (size_t)(p.chunks - 1) * p.chunk_bytes + (size_t)(p.steps - 1) * p.step_bytes + ((size_t)((p.planes - 1) * 4 + p.ntb - 1) * 64 + 64) * 16;
        if (p.dtype == NTK_DT_F16) need = gd_inv_offset(in) + (size_t)T * 4;
        printf(" worth=%d rt=%d ntb=%d planes=%d steps=%d tiles=%d chunks=%d grid=%u block=%u lds=%zu ws=%zu need=%zu least=%d most=%d inside=%d\n", p.worth ? 1 : 0, p.rt, p.ntb,
               p.planes, p.steps, p.tiles, p.chunks, p.grid_x, p.block, p.lds, p.ws_bytes, need, least, worst, inside ? 1 : 0);
    }
    return 0;
}
