// vectorise_pairs.h -- a training batch straight from the packed bases (included by vectorise.hip, inside its anonymous namespace).
//
// idl_gather_pairs_at copies the two rows of a pair out of the resident store feats[n_views][n][4^k] and standardises them.  Here no
// store exists: the rows are made on the spot from what the store was made of -- the packed codes, the invalid mask, the views'
// substitution edits -- and standardised on their way out.  A row is a pure function of those inputs (integer LDS atomics, then the
// correctly rounded float32 quotient count / total), so it has the bits the whole-store kernels gave it, whichever kernel that was.
//   k <= 7: the LDS-histogram design (V2<K, false>): a workgroup per pair counts the un-mutated sequence once (H0), moves the windows
//           around view 0's edits, writes row b, moves them back, does the same for view m + 1 and writes row batch + b.
//   k = 8, 9: the bin-slice design (slices_body): a workgroup per output row, the item taken from the pair list instead of the grid.
// The standardisation is idl_gather_pairs_at's own arithmetic (scaler_device.h).

struct PairArgs {
    const int64_t *pair_idx;
    const int64_t *base;        // device int64 offset into pair_idx (may be NULL = 0)
    int64_t base_add, batch, n_pairs;
    const double *mean, *scale, *inv_scale;     // inv_scale may be NULL: the division itself
    float *y;                   // [2 * batch][4^k] (may be NULL when the planes are given: planes only)
    uint16_t *yh, *yl;          // optional: the batch ALSO as two fp16 planes [2 * batch][4^k] (planes.h, scale 2^X_EXP), as the riding assembly writes them
    int *over;                  // ... and the flag raised when an entry left the planes' range (clamped in the planes)
};

// the pair behind batch row b: false when its place in the pair list lies at or beyond n_pairs (the row is then left alone; so is the
// row of an entry that names no pair of the store: nothing is read for it)
__device__ __forceinline__ bool pair_at(const PairArgs &p, const VecArgs &a, int64_t b, int64_t &m, int64_t &s)
{
    const int64_t at = (p.base ? *p.base : 0) + p.base_add + b;
    if (at < 0 || at >= p.n_pairs) return false;
    const int64_t pair = p.pair_idx[at];
    if (pair < 0 || pair >= a.n * (int64_t)(a.n_views - 1)) return false;
    m = pair / a.n;
    s = pair - m * a.n;
    return true;
}

// four standardised entries of output row `row`, columns c .. c + 3: the fp32 batch and / or its planes (scaler_device.h's gather_tile, restated
// for one quad)
__device__ __forceinline__ void emit4(const PairArgs &p, int64_t row, int64_t f, int64_t c, float4 o)
{
    if (p.y != nullptr) *(float4 *)(p.y + row * f + c) = o;
    if (p.yh != nullptr) {
        constexpr float ps = (float)(1 << idl_planes::X_EXP);
        uint2 h, l;
        if (idl_planes::split4(o.x * ps, o.y * ps, o.z * ps, o.w * ps, h, l) && p.over != nullptr) *p.over = 1;
        *(uint2 *)(p.yh + row * f + c) = h;
        *(uint2 *)(p.yl + row * f + c) = l;
    }
}

__device__ __forceinline__ float4 standardise4(const PairArgs &p, float4 v, int64_t c)
{
    float4 o;
    if (p.inv_scale != nullptr) {
        o.x = idl_dev::std_f32_rcp(v.x, p.mean[c + 0], p.scale[c + 0], p.inv_scale[c + 0]);
        o.y = idl_dev::std_f32_rcp(v.y, p.mean[c + 1], p.scale[c + 1], p.inv_scale[c + 1]);
        o.z = idl_dev::std_f32_rcp(v.z, p.mean[c + 2], p.scale[c + 2], p.inv_scale[c + 2]);
        o.w = idl_dev::std_f32_rcp(v.w, p.mean[c + 3], p.scale[c + 3], p.inv_scale[c + 3]);
    } else {
        o.x = idl_dev::std_f32(v.x, p.mean[c + 0], p.scale[c + 0]);
        o.y = idl_dev::std_f32(v.y, p.mean[c + 1], p.scale[c + 1]);
        o.z = idl_dev::std_f32(v.z, p.mean[c + 2], p.scale[c + 2]);
        o.w = idl_dev::std_f32(v.w, p.mean[c + 3], p.scale[c + 3]);
    }
    return o;
}

constexpr int VP_SC = 160;      // slots staged at a time (10 240 bases, as the whole-store v2 launch)

template <int K>
constexpr int vp_lds_words() { return v2_lds_words(K, false, VP_SC, 0); }     // v2's layout without the views' edit ranges

// second launch-bound argument = waves per SIMD wanted: four workgroups a CU (a batch of 512 pairs puts two on each), which leaves the
// float64 standardisation of the epilogue its registers (six, as vectorise2_kernel asks for, spilled 44 bytes a lane at k = 6)
template <int K>
__global__ __launch_bounds__(64 * V2_WAVES, 4) void vectorise_pairs_kernel(VecArgs a, PairArgs p)
{
    using T = V2<K, false>;
    constexpr int F = T::F, NT = T::NT, SC = VP_SC;
    static_assert(F >= 256, "16-byte row stores from whole histogram quads");
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *hist = lds;                       // F bins + 4 garbage bins
    uint32_t *cod = lds + T::HD;                // (SC + 1) slots x 4 words, slot 0 = halo
    uint32_t *msk = cod + (SC + 1) * 4;         // (SC + 1) slots x 2 words
    uint32_t *ed_lds = msk + (SC + 1) * 2;      // V2_EDIT_CAP edits of the current view
    uint16_t *list_old = (uint16_t *)(ed_lds + V2_EDIT_CAP);
    uint16_t *list_new = list_old + V2_LIST_CAP;
    int64_t *red = (int64_t *)(list_old + 2 * V2_LIST_CAP);   // V2_WAVES partial sums
    const int lane = threadIdx.x;
    auto block_sum = [&](int64_t v) -> int64_t {
        v = wave_sum_i64(v);
        __syncthreads();
        if ((lane & 63) == 0) red[lane >> 6] = v;
        __syncthreads();
        int64_t t = 0;
#pragma unroll
        for (int w = 0; w < V2_WAVES; ++w) t += red[w];
        return t;
    };

    for (int64_t b = blockIdx.x; b < p.batch; b += gridDim.x) {
        int64_t m, s;
        if (!pair_at(p, a, b, m, s)) continue;              // (the same answer in every thread of the workgroup)
        // both rows' edit ranges, and their edits where they fit the LDS cache (<= one a thread), are asked for now: they arrive while the
        // sequence is staged and counted instead of standing in the chain behind it
        int64_t eb2[2] = {0, 0}, ee2[2] = {0, 0};
        if (a.edits != nullptr) {
            eb2[0] = eo_begin(a, s); ee2[0] = eo_end(a, s);
            eb2[1] = eo_begin(a, (m + 1) * a.n + s); ee2[1] = eo_end(a, (m + 1) * a.n + s);
        }
        uint32_t pre2[2] = {0u, 0u};
        static_assert(V2_EDIT_CAP <= 64 * V2_WAVES, "one prefetched edit per thread");
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t c = ee2[h] - eb2[h];
            if (c > 0 && c <= V2_EDIT_CAP && lane < c) pre2[h] = a.edits[eb2[h] + lane];
        }
        const int64_t slot0 = a.slot_off[s];
        const int64_t L = a.lengths[s];
        const int64_t nslots = (L + 63) >> 6;
        const int64_t nsc = (nslots + SC - 1) / SC;

        __syncthreads();
        for (int i = lane; i < T::HD / 4; i += NT) *(uint4 *)(hist + i * 4) = make_uint4(1u, 1u, 1u, 1u);     // IDL_INIT_ONE

        // ---------------- H0: the un-mutated sequence, counted once for both rows (sc 0 last, so a short sequence stays staged)
        uint32_t cnt0 = 0;
        for (int64_t sc = nsc - 1; sc >= 0; --sc) {
            const int nloc = (int)((nslots - sc * SC) < SC ? (nslots - sc * SC) : SC);
            T::stage(a, slot0, sc * SC, nloc, cod, msk, lane);
            cnt0 += T::count_all(cod, msk, nloc, hist, lane);
        }
        const int64_t windows0 = block_sum((int64_t)cnt0);

        for (int half = 0; half < 2; ++half) {
            const int64_t eb = half ? eb2[1] : eb2[0], ee = half ? ee2[1] : ee2[0];     // view 0, then view m + 1
            const int ne = ee > eb ? (int)(ee - eb) : 0;
            const bool mutated = ne > 0 && nsc > 0;
            const bool in_lds = ne <= V2_EDIT_CAP;
            const bool rec = in_lds && nsc == 1 && ne * K <= V2_LIST_CAP && half == 0;      // (nothing is undone after the second row)
            const uint32_t *eg = a.edits + eb;

            // ---------------- forward: hist = H0 - (old windows) + (new windows)
            int dwin = 0;
            if (mutated) {
                if (in_lds) {
                    __syncthreads();
                    if (lane < ne) ed_lds[lane] = half ? pre2[1] : pre2[0];
                    __syncthreads();
                    if (rec) dwin = T::template view_pass<true>(a, (const uint32_t *)ed_lds, ne, slot0, nslots, nsc, SC, L, cod, msk, hist, list_old, list_new, 0xFFFFFFFFu, 1u, lane);
                    else dwin = T::template view_pass<false>(a, (const uint32_t *)ed_lds, ne, slot0, nslots, nsc, SC, L, cod, msk, hist, list_old, list_new, 0xFFFFFFFFu, 1u, lane);
                } else {
                    dwin = T::template view_pass<false>(a, eg, ne, slot0, nslots, nsc, SC, L, cod, msk, hist, list_old, list_new, 0xFFFFFFFFu, 1u, lane);
                }
            }
            const int64_t windows = windows0 + block_sum((int64_t)dwin);
            __syncthreads();

            // ---------------- the row: count / total correctly rounded to float32 (IDL_OUT_FREQ_F32), standardised, one coalesced store
            const int64_t S = windows + (int64_t)F;
            const bool small = S < (1ll << 24);   // then int -> float32 is exact and the float32 division is the float64 division rounded
            const float Sf = (float)S;
            const double Sd = (double)S;
            const int64_t row = (int64_t)half * p.batch + b;
            for (int i4 = lane; i4 < F / 4; i4 += NT) {
                const uint4 h = *(const uint4 *)(hist + i4 * 4);
                float4 f;
                if (small) {
                    f.x = (float)h.x / Sf; f.y = (float)h.y / Sf;
                    f.z = (float)h.z / Sf; f.w = (float)h.w / Sf;
                } else {
                    f.x = (float)((double)h.x / Sd); f.y = (float)((double)h.y / Sd);
                    f.z = (float)((double)h.z / Sd); f.w = (float)((double)h.w / Sd);
                }
                emit4(p, row, F, (int64_t)i4 * 4, standardise4(p, f, (int64_t)i4 * 4));
            }
            __syncthreads();

            // ---------------- undo: hist back to H0 for the pair's other row
            if (mutated && half == 0) {
                if (rec) T::replay(ne * K, hist, list_old, list_new, lane);
                else if (in_lds) (void)T::template view_pass<false>(a, (const uint32_t *)ed_lds, ne, slot0, nslots, nsc, SC, L, cod, msk, hist, list_old, list_new, 1u, 0xFFFFFFFFu, lane);
                else (void)T::template view_pass<false>(a, eg, ne, slot0, nslots, nsc, SC, L, cod, msk, hist, list_old, list_new, 1u, 0xFFFFFFFFu, lane);
            }
        }
        __syncthreads();
    }
}

template <int K>
int launch_vectorise_pairs(VecArgs a, const PairArgs &p, const idl::DeviceInfo &di, hipStream_t st)
{
    const size_t lds = (size_t)vp_lds_words<K>() * 4;
    if ((int)lds > di.max_dyn_lds) {
        idl::set_error("vectorise_pairs: k=%d needs %zu bytes of LDS per workgroup; device allows %d", K, lds, di.max_dyn_lds);
        return IDL_ERR_ARG;
    }
    a.sc_slots = VP_SC;
    const void *fn = (const void *)vectorise_pairs_kernel<K>;
    if (lds > 64 * 1024) IDL_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(vectorise_pairs_kernel<K>, dim3((unsigned)p.batch), dim3(64 * V2_WAVES), lds, st, a, p);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

// ---------------------------------------------------------------- k = 8, 9: one output row per item of the slice kernel's loop
struct SlicePairItems {
    PairArgs p;
    __device__ __forceinline__ int64_t count(const VecArgs &) const { return 2 * p.batch; }
    __device__ __forceinline__ bool item(const VecArgs &a, int64_t it, int64_t row_len, int64_t &s, int &v, int64_t &out_base) const
    {
        int64_t m;
        if (!pair_at(p, a, it < p.batch ? it : it - p.batch, m, s)) return false;
        v = it < p.batch ? 0 : (int)(m + 1);
        out_base = it * row_len;                  // output row `it` of y and of the planes
        return true;
    }
    __device__ __forceinline__ void store_f32(const VecArgs &, int64_t o, int64_t col, float4 f) const
    {
        emit4(p, 0, 0, o, standardise4(p, f, col));
    }
};

// (second launch-bound argument = waves per SIMD: the launcher's two workgroups a CU are 4; without it the planes' split took the kernel to 135
//  VGPRs, one workgroup a CU, and the launch from 57 to 92 us at k = 8)
template <int K>
__global__ __launch_bounds__(SL_NT, 2 * SL_WG_PER_CU) void vectorise_pairs_slices_kernel(VecArgs a, PairArgs p)
{
    slices_body<K>(a, nullptr, SlicePairItems{p});
}

template <int K>
int launch_vectorise_pairs_slices(const VecArgs &a, const PairArgs &p, const idl::DeviceInfo &di, hipStream_t st)
{
    const size_t lds = (size_t)SL_LDS_WORDS * 4;
    if ((int)lds > di.max_dyn_lds) {
        idl::set_error("vectorise_pairs: k=%d needs %zu bytes of LDS per workgroup; device allows %d", K, lds, di.max_dyn_lds);
        return IDL_ERR_ARG;
    }
    const void *fn = (const void *)vectorise_pairs_slices_kernel<K>;
    IDL_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    int64_t grid = (int64_t)di.cus * SL_WG_PER_CU;
    if (grid > 2 * p.batch) grid = 2 * p.batch;
    hipLaunchKernelGGL(vectorise_pairs_slices_kernel<K>, dim3((unsigned)grid), dim3(SL_NT), lds, st, a, p);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

// the bounds of the kernels above, as idl_vectorise_pairs_supported states them
inline bool vectorise_pairs_shape_ok(int k, int64_t f, int64_t batch, int64_t max_len)
{
    // 4 <= k <= 9 plain k-mer rows; one workgroup per pair in the grid's x; edit positions and window counts as the vectoriser packs them
    return k >= 4 && k <= IDL_MAX_K && f == (1ll << (2 * k)) && batch >= 0 && batch <= 0x3FFFFFFFll && max_len >= 0 && max_len < (1ll << 30);
}
