// tests/kv_layout_check.cpp -- prints what ntransformer_amd/csrc/kv_layout.h computes, for tests/test_kv_layout_cpu.py to compare with the built
// library and the Python mirror.  Host C++ only; includes nothing of the project but that header.
// Arguments, in order: "S,NKV,HD" names a geometry (max_seq, n_kv_heads, head_dim) and prints
//     geom S NKV HD <f16 layer elements> <q8 layer bytes> <q8 scale-plane offset>
// "POS0+N" prints, for the last geometry named,
//     rows POS0 N <f16 byte off> <f16 bytes> <q8 quant off> <q8 quant bytes> <q8 scale off> <q8 scale bytes>
#include <cstdio>
#include "../ntransformer_amd/csrc/kv_layout.h"

static_assert(ntk::kv_q8_layer_bytes(1, 1, 128) == 256 && ntk::kv_q8_layer_bytes(4096, 8, 128) == 4096 * 1088, "usable in constant expressions");

int main(int argc, char** argv) {
    ntk::KvGeom g{1, 0, 0, 0};
    for (int i = 1; i < argc; ++i) {
        int a, b, c;
        if (sscanf(argv[i], "%d,%d,%d", &a, &b, &c) == 3) {
            g = ntk::KvGeom{1, a, b, c};
            printf("geom %d %d %d %zu %zu %zu\n", a, b, c, ntk::kv_f16_layer_elems(g.max_seq, g.per()), ntk::kv_q8_layer_bytes(a, b, c),
                   ntk::kv_q8_scale_offset(g.max_seq, g.per()));
        } else if (sscanf(argv[i], "%d+%d", &a, &b) == 2) {
            const ntk::KvRange f = ntk::kv_f16_rows(g.per(), a, b), q = ntk::kv_q8_quant_rows(g.per(), a, b), s = ntk::kv_q8_scale_rows(g.max_seq, g.per(), a, b);
            printf("rows %d %d %zu %zu %zu %zu %zu %zu\n", a, b, f.off, f.bytes, q.off, q.bytes, s.off, s.bytes);
        } else {
            fprintf(stderr, "kv_layout_check: bad argument '%s'\n", argv[i]);
            return 2;
        }
    }
    return 0;
}
