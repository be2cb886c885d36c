// tests/gemm_plan_check.cpp -- prints what ntransformer_amd/csrc/gemm_f16_plan.h plans, for tests/test_gemm_plan_cpu.py to compare with the table recorded
// from the launch code before the plan had a header of its own (tests/golden/gemm_f16_plans.txt).  Host C++ only; includes nothing of the project but that header.
// Each argument "FMT:T:IN:ROWS[,ROWS[,ROWS]]:FULL" (FMT = Q8_0 Q4_0 Q4_K Q5_K Q6_K Q4_K_RP Q5_K_RP Q6_K_RP) prints one line:
//     FMT T=. in=. rows=.,. full=. : status=-2                                          (a shape the format cannot take)
//     FMT T=. in=. rows=.,. full=. : form=kslice|small|chunk rt ntb cw al pf nsplit per_split jobs waves grid=x,y block lds tiles chunks row_bytes
//                                    seg=tile0,tiles16,w_last,p2_off[,part_off] per matrix (part_off: the forms with a partial-sum area)
#include <cstdio>
#include <cstring>
#include "../ntransformer_amd/csrc/gemm_f16_plan.h"

static_assert(ntk::ws_chunk_bytes(4096) % 256 == 0 && ntk::gb_lds_bytes<NTK_DT_Q8_0, 2, 1>() <= ntk::GB_LDS_WG, "usable in constant expressions");

static bool plan_for(const char* fmt, const int* rows, int nseg, int T, int in, bool full, ntk::GemmPlan& p) {
    const ntk::GemmTune tune;
    if (!strcmp(fmt, "Q8_0")) p = ntk::gemm_f16_plan<NTK_DT_Q8_0>(rows, nseg, T, in, full, tune);
    else if (!strcmp(fmt, "Q4_0")) p = ntk::gemm_f16_plan<NTK_DT_Q4_0>(rows, nseg, T, in, full, tune);
    else if (!strcmp(fmt, "Q4_K")) p = ntk::gemm_f16_plan<NTK_DT_Q4_K>(rows, nseg, T, in, full, tune);
    else if (!strcmp(fmt, "Q5_K")) p = ntk::gemm_f16_plan<NTK_DT_Q5_K>(rows, nseg, T, in, full, tune);
    else if (!strcmp(fmt, "Q6_K")) p = ntk::gemm_f16_plan<NTK_DT_Q6_K>(rows, nseg, T, in, full, tune);
    else if (!strcmp(fmt, "Q4_K_RP")) p = ntk::gemm_f16_plan<NTK_DT_Q4_K + ntk::GB_RP>(rows, nseg, T, in, full, tune);
    else if (!strcmp(fmt, "Q5_K_RP")) p = ntk::gemm_f16_plan<NTK_DT_Q5_K + ntk::GB_RP>(rows, nseg, T, in, full, tune);
    else if (!strcmp(fmt, "Q6_K_RP")) p = ntk::gemm_f16_plan<NTK_DT_Q6_K + ntk::GB_RP>(rows, nseg, T, in, full, tune);
    else return false;
    return true;
}

int main(int argc, char** argv) {
    static const char* const FORM[] = {"kslice", "small", "chunk"};
    for (int a = 1; a < argc; ++a) {
        char fmt[16];
        int T, in, full, rows[3], used = 0;
        if (sscanf(argv[a], "%15[^:]:%d:%d:%n", fmt, &T, &in, &used) != 3) { fprintf(stderr, "gemm_plan_check: bad argument '%s'\n", argv[a]); return 2; }
        int nseg = sscanf(argv[a] + used, "%d,%d,%d", &rows[0], &rows[1], &rows[2]);
        const char* tail = strrchr(argv[a], ':');
        ntk::GemmPlan p;
        if (nseg < 1 || sscanf(tail, ":%d", &full) != 1 || !plan_for(fmt, rows, nseg, T, in, full != 0, p)) {
            fprintf(stderr, "gemm_plan_check: bad argument '%s'\n", argv[a]);
            return 2;
        }
        printf("%s T=%d in=%d rows=", fmt, T, in);
        for (int i = 0; i < nseg; ++i) printf("%s%d", i ? "," : "", rows[i]);
        printf(" full=%d :", full);
        if (p.status != NTK_OK) { printf(" status=%d\n", p.status); continue; }
        printf(" form=%s rt=%d ntb=%d cw=%d al=%d pf=%d nsplit=%d per_split=%d jobs=%d waves=%d grid=%u,%u block=%u lds=%zu tiles=%d chunks=%d row_bytes=%u",
               FORM[p.form], p.rt, p.ntb, p.cw, (int)p.al, (int)p.pf, p.nsplit, p.per_split, p.jobs, p.waves, p.grid_x, p.grid_y, p.block, p.lds, p.tiles,
               p.chunks, p.row_bytes);
        for (int i = 0; i < nseg; ++i) {
            printf(" seg=%d,%d,%u,%u", p.seg[i].tile0, p.seg[i].tiles16, p.seg[i].w_last, p.seg[i].p2_off);
            if (p.form != ntk::GEMM_FORM_SMALL) printf(",%zu", p.seg[i].part_off);
        }
        printf("\n");
    }
    return 0;
}
