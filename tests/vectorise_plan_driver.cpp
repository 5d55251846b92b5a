// Stand-alone driver of csrc/vectorise_plan.h for tests/test_vectorise_plan.py (plain g++, no HIP).
//   driver            : one case per line of stdin --
//                       k mode init out_kind n_views has_edits n max_len cus lds_per_cu max_dyn_lds per_cu IDELUCS_DEV-or-"-"
//                       (per_cu: the runtime's occupancy answer, used where the plan leaves workgroups per CU open: v1 / v2)
//                       -> the launcher's IDELUCS_DEBUG line, then the plan's fields and the LDS bytes the layout functions give for them
//   driver --table    : DESIGN.md 4.1's routing table (an MI355X: 256 CUs, 160 KiB of LDS each), as markdown
#include <string.h>

#include "vectorise_plan.h"

static const char *kernel_name(int kernel)
{
    static const char *nm[] = {"none", "v1", "v2", "v2/16-bit bins", "v3", "v4", "slices"};
    return nm[kernel];
}

// the first pass's dynamic LDS from the layout functions alone, given the kernel arguments the plan sets
static int layout_bytes(const VecShape &s, const VecPlan &p)
{
    switch (p.kernel) {
    case IDL_VEC_V1: return v1_lds_words(s.k) * 4;
    case IDL_VEC_V2: return v2_lds_words(s.k, false, p.sc_slots, s.n_views) * 4;
    case IDL_VEC_V2_B16: return v2_lds_words(s.k, true, p.sc_slots, s.n_views) * 4;
    case IDL_VEC_V3: return v3_lds_words(s.k, p.copies_log2, p.sc_slots, p.ecap, p.lcap) * 4;
    case IDL_VEC_V4: return v4_slice_words(s.k, p.copies_log2, p.v3_sc, p.ecap) * 4 * p.waves;
    case IDL_VEC_SLICES: return SL_LDS_WORDS * 4;
    }
    return -1;
}

static void table()
{
    const VecDevice d{256, 160 * 1024, 160 * 1024};
    struct Row { const char *what; VecShape s; const char *dev; };
    const int64_t n = 100000;
    const Row rows[] = {
        {"k = 1..3, 7 (here 3): any mode", {3, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 10000}, ""},
        {"k = 7", {7, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 10000}, ""},
        {"k = 4, <= 12 288 bases, <= 8 views", {4, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 10000}, ""},
        {"k = 5, the same", {5, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 10000}, ""},
        {"k = 6, CGR / canonical rows, the same", {6, IDL_MODE_CGR, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 10000}, ""},
        {"k = 6, plain rows, <= 131 072 bases", {6, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 10000}, ""},
        {"k = 6, plain rows, no edits", {6, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 1, 0, n, 10000}, ""},
        {"k = 4, 12 289 .. 131 072 bases (here 20 000)", {4, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 20000}, ""},
        {"k = 5, 30 000 bases", {5, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 30000}, ""},
        {"k = 6, 40 000 bases: v3's LDS passes 80 KB", {6, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 40000}, ""},
        {"k = 4..6, CGR / canonical, > 12 288 bases", {5, IDL_MODE_CGR, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 20000}, ""},
        {"k = 4..6, no length bound (max_len = 0)", {6, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 0}, ""},
        {"k = 4..6, float64 rows", {6, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F64, 4, 1, n, 10000}, ""},
        {"k = 4..6, more than 8 views", {6, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 9, 1, n, 10000}, ""},
        {"k <= 7, IDL_INIT_FROM_OUT", {6, IDL_MODE_KMER, IDL_INIT_FROM_OUT, IDL_OUT_COUNTS_I32, 1, 0, 1, 10000}, ""},
        {"k = 8, 9", {8, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 10000}, ""},
        {"`vec=1`", {5, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 10000}, "vec=1"},
        {"`vec=2` (`vec=4` where v4 declines: the same)", {5, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 10000}, "vec=2"},
        {"`vec=3`", {5, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 10000}, "vec=3"},
        {"`vec=2,bins=16`, <= 65 000 bases", {6, IDL_MODE_KMER, IDL_INIT_ONE, IDL_OUT_FREQ_F32, 4, 1, n, 10000}, "vec=2,bins=16"},
    };
    printf("| shape (100 000 sequences of <= 10 000 bases, 4 views with edits, float32 rows unless it says otherwise) | kernel | LDS a workgroup | workgroups / CU | second pass |\n|---|---|---|---|---|\n");
    for (const Row &r : rows) {
        setenv("IDELUCS_DEV", r.dev, 1);
        const VecPlan p = plan_vectorise(r.s, d, read_vec_knobs());
        char inst[96] = "", per_cu[64] ="the runtime's occupancy answer, <= 16", redo[96] = "-";
        if (p.kernel == IDL_VEC_V4) snprintf(inst, sizeof(inst), " (%d waves, %d copies%s)", p.waves, 1 << p.copies_log2, p.other_modes ? ", CGR / canonical instance" : "");
        if (p.kernel == IDL_VEC_V3) snprintf(inst, sizeof(inst), " (%d copies, tables for %d edits / %d pairs)", 1 << p.copies_log2, p.ecap, p.lcap);
        if (p.wg_per_cu) snprintf(per_cu, sizeof(per_cu), "%d", p.wg_per_cu);
        if (p.redo) snprintf(redo, sizeof(redo), "v2, %d B, %d workgroups", p.redo_lds_bytes, p.redo_grid);
        printf("| %s | %s%s | %d B | %s | %s |\n", r.what, kernel_name(p.kernel), inst, p.lds_bytes, per_cu, redo);
    }
}

int main(int argc, char **argv)
{
    if (argc > 1 && strcmp(argv[1], "--table") == 0) { table(); return 0; }
    VecShape s;
    VecDevice d;
    long long n, max_len;
    int per_cu;
    char dev[512];
    while (scanf("%d %d %d %d %d %d %lld %lld %d %d %d %d %511s", &s.k, &s.mode, &s.init, &s.out_kind, &s.n_views, &s.has_edits, &n, &max_len,
                 &d.cus, &d.lds_per_cu, &d.max_dyn_lds, &per_cu, dev) == 13) {
        s.n = n;
        s.max_len = max_len;
        if (strcmp(dev, "-") == 0) unsetenv("IDELUCS_DEV");
        else setenv("IDELUCS_DEV", dev, 1);
        VecPlan p = plan_vectorise(s, d, read_vec_knobs());
        if (p.lds_bytes > d.max_dyn_lds) printf("too large\n");
        else {
            if (p.wg_per_cu == 0) vec_plan_occupancy(p, s, d, per_cu);
            char line[256];
            vec_plan_line(line, sizeof(line), s.k, p);
            printf("%s\n", line);
        }
        printf("kernel=%d rl=%d om=%d diag=%d threads=%d lds=%d layout=%d grid=%d redo=%d redo_sc=%d redo_lds=%d redo_layout=%d redo_grid=%d\n", p.kernel, p.copies_log2,
               p.other_modes, p.diag, p.threads, p.lds_bytes, layout_bytes(s, p), p.grid, p.redo, p.redo_sc_slots, p.redo_lds_bytes,
               v2_lds_words(s.k, false, 160, s.n_views) * 4, p.redo_grid);
    }
    return 0;
}
