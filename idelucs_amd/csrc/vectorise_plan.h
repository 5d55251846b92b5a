// vectorise_plan.h -- which kernel vectorises which input, with how much LDS, and what cleans up behind it: the vectoriser's whole launch policy
// as ONE pure function.  Host-compilable (no HIP header): vectorise.hip launches what plan_vectorise says, idl_vectorise_plan reports it, and
// tests/test_vectorise_plan.py replays recorded launches through it on a CPU.
//
//   k = 8, 9                                                   -> slices (vectorise_slices.h)
//   the hot shape: k = 4..6, fresh histograms, int32 / float32 rows, <= 8 views, a length bound, and
//     k = 4, 5 (any mode) or k = 6 (CGR / canonical), <= 12 288 bases, >= 4 waves' slices in a CU's LDS   -> v4, a wave per sequence
//     plain k-mer rows, <= 64 * 2048 bases, <= 80 KB of LDS                                               -> v3, a workgroup per sequence
//     both leave the sequences that overflow their LDS tables to a second pass on v2
//   IDL_INIT_FROM_OUT (a per-view start), or IDELUCS_DEV=vec=1 -> v1
//   everything else                                            -> v2 (IDELUCS_DEV=bins=16: two 16-bit bins a word)
// IDELUCS_DEV=vec=N keeps the kernels above vN out (the cross-check tests): 4 and 3 are the defaults of their own stages, so vec=4 does NOT fall to v3.
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "../../include/idelucs_hip.h"
#include "dev_env.h"
#include "vectorise_layout.h"

struct VecShape { int k, mode, init, out_kind, n_views, has_edits; int64_t n, max_len; };
struct VecDevice { int cus, lds_per_cu, max_dyn_lds; };        // idl::DeviceInfo's three numbers
typedef idl_vectorise_plan_t VecPlan;                          // (include/idelucs_hip.h: the fields, one by one)

// the vectoriser's IDELUCS_DEV keys, read once per call
struct VecKnobs {
    bool vec_set = false;
    int vec = 0;                  // vec=N
    int sc_slots = 160;           // v1 / v2: 10240 bases staged at a time (cfg2's 10 kbp in one super-chunk)
    bool bins16 = false;          // bins=16
    int v3_ec = -1, v3_lc = -1;   // v3_ec / v3_lc: the LDS tables' capacities (< 0: not set; each kernel has its own upper bound)
    int v3_rl = 4, v4_rl = 2;     // log2 of v3_copies / v4_copies (k = 4)
    bool dbg = false;             // vec_dbg
    int ablate = 0;               // vec_ablate
    int want(int def) const { return vec_set ? vec : def; }
};

inline VecKnobs read_vec_knobs()
{
    VecKnobs kn;
    if (const char *e = idl::dev_env("vec")) { kn.vec_set = true; kn.vec = atoi(e); }
    kn.sc_slots = idl::dev_env_int("sc_slots", 160, 1, 4096);
    if (const char *e = idl::dev_env("bins")) kn.bins16 = atoi(e) == 16;
    if (const char *e = idl::dev_env("v3_ec")) kn.v3_ec = atoi(e);
    if (const char *e = idl::dev_env("v3_lc")) kn.v3_lc = atoi(e);
    // v3, k = 4: copies of the histogram the count goes to: 16 by default -- measured at 100 000 x 10 kbp, 4 views (round 5): 0.708 ms
    // with 16 (four workgroups per CU), 0.714 with 8, 0.844 with 32 (conflict-free, but 41 KB of LDS: three per CU); v2: 1.393
    if (const char *e = idl::dev_env("v3_copies")) { const int t = atoi(e); kn.v3_rl = t == 32 ? 5 : (t == 8 ? 3 : 4); }
    // v4, k = 4: copies of the histogram a wave counts into: 4 -- measured at 100 000 x 10 kbp, 4 views, one box (round 6): no edits / philox edits
    // 0.351 / 0.649 ms with 4, 0.349 / 0.738 with 8, 0.453 / 1.025 with 16 (fewer waves fit); v3 on the same box: 0.621 / 0.725
    if (const char *e = idl::dev_env("v4_copies")) { const int t = atoi(e); kn.v4_rl = t == 16 ? 4 : (t == 8 ? 3 : (t == 1 ? 0 : 2)); }
    // (k = 5 with the count in 4 / 8 copies was measured too (round 5): 0.904 / 1.139 ms against 0.804 without -- folding
    //  1024 bins x copies costs more than the conflicts it saves; bit-identical rows: k = 5, 6 take no copies)
    kn.dbg = idl::dev_env("vec_dbg") != nullptr;
    if (const char *e = idl::dev_env("vec_ablate")) kn.ablate = atoi(e);
    return kn;
}

inline VecPlan plan_vectorise(const VecShape &s, const VecDevice &d, const VecKnobs &kn)
{
    VecPlan p{};
    const int K = s.k;
    // the first pass: kernel and instance, a workgroup's threads and LDS, workgroups per CU (0: the runtime's answer) and the grid they make, <= `work`
    const auto first_pass = [&](int kernel, int rl, int threads, int lds, int per_cu, int64_t work) {
        p.kernel = kernel; p.copies_log2 = rl; p.threads = threads; p.lds_bytes = lds; p.wg_per_cu = per_cu;
        p.grid = (int)((int64_t)d.cus * per_cu > work ? work : (int64_t)d.cus * per_cu);
    };
    if (K >= 8) {                                  // the histogram exceeds one CU's LDS
        first_pass(IDL_VEC_SLICES, 0, SL_NT, SL_LDS_WORDS * 4, SL_WG_PER_CU, s.n * s.n_views);
        return p;
    }
    const bool om = s.mode == IDL_MODE_CGR || s.mode == IDL_MODE_CANONICAL;
    // v3 / v4 take the hot shape only: k = 4..6, <= 8 views, every sequence within the staged slots (the host's length bound says so), fresh
    // histograms, int32 or float32 rows.  Everything else stays on v2 / v1.
    const bool hot = K >= 4 && K <= 6 && s.init != IDL_INIT_FROM_OUT && s.out_kind != IDL_OUT_FREQ_F64 && s.n_views <= V3_MAXV && s.max_len > 0 &&
                     s.n <= 0x7F000000ll;
    const int sc = (int)((s.max_len + 63) / 64);
    const auto second_pass = [&](int redo) {       // v2 on the sequences the first pass left alone; exits at once when there are none
        p.redo = redo; p.redo_sc_slots = 160; p.redo_v3_sc = sc;
        p.redo_lds_bytes = v2_lds_words(K, false, p.redo_sc_slots, s.n_views) * 4;
        p.redo_grid = (int)((int64_t)d.cus * 4 > s.n ? s.n : (int64_t)d.cus * 4);
    };
    // v4: a wave per sequence, when every sequence fits its wave's slice of LDS (<= 12 288 bases).  Plain rows at k = 6 are v3's: bound by the write
    // stream there.  (k = 6, CGR / canonical: 2.29 / 4.99 ms at 100 000 x 10 kbp x 4 views against v2's 3.05 / 7.53.  The collapse is latency-bound -- 4096
    // bins x 4 views a sequence walked by one wave in 64 turns, twice --, not bank- or instruction-bound: summing the pairs in place in a skewed,
    // conflict-free order (lane l of turn t takes b = l | ((l + t) mod 64) << 6) and restoring them by a third walk was built and measured: 6.0 ms at
    // k = 6, no change at k = 4 / 5; rc(b) from per-lane and per-turn halves (no bit reversal in the loop) measured too: 5.1 ms -- a walk costs ~1.3 ms
    // whatever its body: 64 dependent turns of LDS latency at two waves a SIMD)
    if (hot && kn.want(4) == 4 && !(K == 6 && !om) && s.max_len <= 64 * 64 * V4_SR) {
        const int rl = K == 4 ? kn.v4_rl : 0;
        int ec = !s.has_edits ? 0 : (((int)(s.max_len * 35 / 1000) + 64) * s.n_views / 4 + 7) & ~7;      // edits of all views: 3.5 % of the bases + slack for four views, scaled
        if (ec > 64 * V4_FR) ec = 64 * V4_FR;
        if (kn.v3_ec >= 0 && kn.v3_ec <= 64 * V4_FR) ec = kn.v3_ec & ~7;
        const int slice = v4_slice_words(K, rl, sc, ec);
        // as many waves a workgroup as its CU's LDS holds slices (one workgroup per CU: nothing is shared between the waves but the CU)
        int waves = (d.lds_per_cu - 2048) / (slice * 4);
        if (waves > V4_MAX_WAVES) waves = V4_MAX_WAVES;
        if (waves >= 4 && slice * 4 * waves <= d.max_dyn_lds) {           // (fewer: long sequences, v3 / v2)
            first_pass(IDL_VEC_V4, rl, 64 * waves, slice * 4 * waves, 1, (s.n + waves - 1) / waves);
            p.other_modes = om || K == 6;
            p.waves = waves;
            p.sc_slots = p.v3_sc = sc;
            p.ecap = ec;
            second_pass(2);
            return p;
        }
    }
    // v3: a workgroup per sequence, staged by LDS-DMA one sequence ahead.  k = 4 counts into 2^RL copies of its 1 KB histogram (V3<K, RL>): RL = 5 is
    // conflict-free and fits three workgroups per CU at 10 kbp, RL = 4 four.
    if (hot && kn.want(3) == 3 && s.mode == IDL_MODE_KMER && s.max_len <= 64 * 2048) {
        const int rl = K == 4 ? kn.v3_rl : 0;
        // LDS tables for the edits of all views and their K windows each: at least 3.5 % of the bases + slack, and whatever else
        // fits at four workgroups per CU (an edit costs 2 + K words: two staging sets and the list); IDELUCS_DEV=v3_ec / v3_lc override
        int ec = (int)(s.max_len * 35 / 1000) + 64, lc;
        {
            const int fixed = v3_lds_words(K, rl, sc, 0, 0);
            int wgs = 4;                                  // workgroups per CU the tables are sized for: four, or as many as the fixed part + the minimum leaves
            while (wgs > 2 && ((d.lds_per_cu / wgs - 1024) / 4 - fixed) / (2 + K) < ec) --wgs;
            const int fit = ((d.lds_per_cu / wgs - 1024) / 4 - fixed) / (2 + K);
            if (fit > ec) ec = fit > 4096 ? 4096 : fit;
        }
        if (kn.v3_ec >= 0 && kn.v3_ec <= 16384) ec = kn.v3_ec;
        ec &= ~7;
        lc = ec * K;
        if (kn.v3_lc >= 0 && kn.v3_lc <= 65536) lc = kn.v3_lc;
        if (!s.has_edits) { ec = 0; lc = 0; }
        const int lds = v3_lds_words(K, rl, sc, ec, lc) * 4;
        if (lds <= d.max_dyn_lds && lds <= 80 * 1024) {  // (more: fewer than two workgroups per CU, v2's chunked staging is the better fit)
            // workgroups per CU by LDS, with 1 KB of slack each (measured: five 32 032-byte workgroups do NOT become resident
            // together although 5 x 32 032 < 160 KB and the occupancy query says 5 -- the fifth ran after the others)
            const int fit = d.lds_per_cu / (lds + 1024);
            first_pass(IDL_VEC_V3, rl, V3_NT, lds, fit > 4 ? 4 : (fit < 1 ? 1 : fit), s.n);       // (four: 8 waves per workgroup, <= 64 registers: 32 waves per CU)
            p.diag = kn.dbg;
            p.sc_slots = sc;
            p.ecap = ec;
            p.lcap = lc;
            p.chunk = 2;
            p.ablate = kn.ablate;
            second_pass(1);
            return p;
        }
    }
    const bool v1 = s.init == IDL_INIT_FROM_OUT || kn.want(0) == 1;      // accumulate-on-top needs a per-view start: the single-pass kernel
    // 16-bit bins are possible while no count can reach 65536 (count <= max_len + 1).  Measured on MI355X (cfg2): 8
    // workgroups/CU with 16-bit bins (64 VGPRs, 80 B/lane of spill) run 2.16 ms, 6 workgroups/CU with 32-bit bins
    // (79 VGPRs) 1.98 ms -- so 32-bit is the default and 16-bit an opt-in experiment (IDELUCS_DEV=bins=16).
    const bool b16 = kn.bins16 && !v1 && s.max_len > 0 && s.max_len <= 65000;
    if (v1) first_pass(IDL_VEC_V1, 0, 64, v1_lds_words(K) * 4, 0, s.n);
    else first_pass(b16 ? IDL_VEC_V2_B16 : IDL_VEC_V2, 0, 64 * V2_WAVES, v2_lds_words(K, b16, kn.sc_slots, s.n_views) * 4, 0, s.n);
    p.sc_slots = kn.sc_slots;
    p.ablate = kn.ablate;
    return p;                                      // wg_per_cu = 0: the runtime's occupancy answer, vec_plan_occupancy() below
}

// v1 / v2: the launcher's occupancy query finishes the plan
inline void vec_plan_occupancy(VecPlan &p, const VecShape &s, const VecDevice &d, int per_cu)
{
    p.wg_per_cu = per_cu > 16 ? 16 : (per_cu < 1 ? 1 : per_cu);
    p.grid = (int)((int64_t)d.cus * p.wg_per_cu > s.n ? s.n : (int64_t)d.cus * p.wg_per_cu);
}

// the IDELUCS_DEBUG line of a first-pass launch
inline void vec_plan_line(char *buf, size_t size, int k, const VecPlan &p)
{
    if (p.kernel == IDL_VEC_SLICES) snprintf(buf, size, "[idl] vectorise k=%d slices lds=%d B, %d workgroups", k, p.lds_bytes, p.grid);
    else if (p.kernel == IDL_VEC_V4)
        snprintf(buf, size, "[idl] vectorise k=%d v4 (a wave per sequence) lds=%d B a workgroup of %d waves (copies %d, staged slots %d, edits %d, pairs %d) -> %d workgroups/CU",
                 k, p.lds_bytes, p.waves, 1 << p.copies_log2, p.v3_sc, p.ecap, p.lcap, p.wg_per_cu);
    else if (p.kernel == IDL_VEC_V3)
        snprintf(buf, size, "[idl] vectorise k=%d v3 lds=%d B (histogram copies %d, staged slots %d, edits %d, pairs %d) -> %d workgroups/CU",
                 k, p.lds_bytes, 1 << p.copies_log2, p.sc_slots, p.ecap, p.lcap, p.wg_per_cu);
    else
        snprintf(buf, size, "[idl] vectorise k=%d %s lds=%d B -> %d workgroups/CU", k,
                 p.kernel == IDL_VEC_V1 ? "v1" : (p.kernel == IDL_VEC_V2_B16 ? "v2/16-bit bins" : "v2/32-bit bins"), p.lds_bytes, p.wg_per_cu);
}
