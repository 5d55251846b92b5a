// vectorise_layout.h -- the LDS layout constants of the vectoriser's kernels and ONE word count per kernel (included by vectorise_plan.h, and
// through it by vectorise.hip).  Host-compilable: no HIP header, so the plan and its CPU test see the sizes the kernels carve.
#pragma once

constexpr int STAGE_DWORDS = 256 + 128;  // v1: 64 lanes x (4 code words + 2 mask words)

constexpr int V2_LIST_CAP = 768;   // (edit, window) pairs recorded per view for a replay-undo
constexpr int V2_EDIT_CAP = 192;   // edits of a view preloaded into LDS
constexpr int V2_WAVES = 4;        // wavefronts per sequence

constexpr int V3_MAXV = 8;                      // views
constexpr int V3_META = 8 + 4 * V3_MAXV;        // dwords of a meta ring entry: slot_off[s], slot_off[s+1], lengths[s], pad; per view edit_off[v*n+s], [..+1]
constexpr int V3_VT = 4;                        // dwords of a view-table row: edits, first edit's index in LDS, first pair's index in the list, spare
constexpr int V3_VTAB = (V3_MAXV + 1) * V3_VT;  // row 0 = header: flags (1 fast, 2 edits staged), total pairs, staged slots, clamped length
constexpr int V3_NC = 384;                      // compute threads (6 waves)
constexpr int V3_MW = 2;                        // memory waves, each holding 1 / V3_MW of a row
constexpr int V3_NT = V3_NC + 64 * V3_MW;

constexpr int V4_MAX_WAVES = 12;                // waves of a workgroup: as many as the slices of LDS allow (the plan decides)
constexpr int V4_SR = 3;                        // rounds of 64 slots a sequence may take (12 288 bases); longer inputs stay on v3 / v2
constexpr int V4_FR = 10;                       // rounds of 64 edits (ALL views of a sequence, one after the other) prefetched into registers; more: second pass

constexpr int SL_BITS = 14;                 // k = 8, 9: log2 of the bins of a slice
constexpr int SL_BINS = 1 << SL_BITS;       // 64 KiB of uint32 bins
constexpr int SL_NT = 512;                  // threads of a workgroup (8 wavefronts)
constexpr int SL_SC = 320;                  // slots (64 bases) staged at a time: 20 480 bases, 7.5 KiB
constexpr int SL_LDS_WORDS = SL_BINS + (SL_SC + 1) * 6 + 2 * (SL_NT / 64);
constexpr int SL_WG_PER_CU = 2;             // residency the plan assumes: 2 x 73 KiB of the CU's 160 KiB

// histogram words: V2<K, B16>::F / ::HD (4 garbage bins behind the bins, kept a multiple of 4) and V3<K, RL>::HC / ::HD (2^RL copies in front)
constexpr int vec_bins(int k) { return 1 << (2 * k); }
constexpr int v2_hist_words(int k, bool b16) { return b16 ? (vec_bins(k) / 2 + 4) & ~3 : vec_bins(k) + 4; }
constexpr int v3_copy_words(int k, int rl) { return rl ? (vec_bins(k) + 4) << rl : 0; }
constexpr int v3_hist_words(int k, int rl) { return v3_copy_words(k, rl) + v2_hist_words(k, false); }

// a staged super-chunk: sc slots + the halo slot, 4 code words + 2 mask words each
constexpr int staged_words(int sc) { return (sc + 1) * 6; }

// dynamic LDS of a workgroup, in words, in the order the kernels carve it
constexpr int v1_lds_words(int k) { return vec_bins(k) + STAGE_DWORDS; }
// histogram | staged super-chunk | a view's edits | old / new pair lists (16-bit) | V2_WAVES partial sums (64-bit) | edit ranges of the views (2 x 64-bit)
constexpr int v2_lds_words(int k, bool b16, int sc, int n_views)
{
    return v2_hist_words(k, b16) + staged_words(sc) + V2_EDIT_CAP + V2_LIST_CAP + 2 * V2_WAVES + 4 * n_views;
}
constexpr int v3_set_words(int sc, int ec) { return staged_words(sc) + ec; }         // one staging set: the super-chunk and the edits of all views
// copies + histogram | two staging sets | lc pairs | ring of 3 meta entries | two view tables | 16 counters | 4 queue words
constexpr int v3_lds_words(int k, int rl, int sc, int ec, int lc)
{
    return v3_hist_words(k, rl) + 2 * v3_set_words(sc, ec) + lc + 3 * V3_META + 2 * V3_VTAB + 16 + 4;
}
// v4: ONE wave's slice -- copies | histogram + 4 garbage bins | staged sequence | edits of all views
constexpr int v4_slice_words(int k, int rl, int sc, int ec) { return (v3_copy_words(k, rl) + (vec_bins(k) + 4) + staged_words(sc) + ec + 3) & ~3; }
