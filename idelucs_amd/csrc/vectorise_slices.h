// vectorise_slices.h -- the vectoriser for k = 8 and 9 (included by vectorise.hip, inside its anonymous namespace).
//
// 4^8 / 4^9 uint32 bins are 256 KiB / 1 MiB: the histogram of a sequence does not fit one CU's LDS, so the row is produced in
// SLICES of 2^14 output bins (64 KiB of LDS, two workgroups per CU).  A workgroup owns one (sequence, view) item at a time:
//   * the packed codes and the invalid mask are staged in LDS one super-chunk (SL_SC slots + a halo slot) at a time and the view's
//     substitution edits are applied to the staged copy (XOR on the 2-bit codes / set-N, as vectorise_kernel does);
//   * for every slice the windows are walked once; a window is mapped to its OUTPUT bin (k-mer index; CGR pixel; canonical
//     representative min(b, rc(b))) and counted iff that bin falls into the slice -- LDS atomics on integers, so a row is a pure
//     function of its inputs whatever the scheduling;
//   * the slice is finished with the epilogue arithmetic of the k <= 7 kernels and stored -- the only global write.
// Because the histogram is kept in output order, IDL_INIT_FROM_OUT starts a slice from the caller's slice of the row, and a CGR
// row needs no permutation at store time.
// Normalisation: a plain / CGR row's total is init * 4^k + (valid windows), known after the first walk.  A canonical row is divided
// by the sum of its TRUNCATED bins (utils.py:208-221), which needs every slice: the frequency kinds of the canonical mode sweep
// the slices twice (first the sum, then the row).  Canonical bins hold c[b] + c[rc(b)] directly (a palindrome: c[b]), so the value
// is h / 2 (a palindrome: h); the output position of bin b is rank_tab[b / 64] (canonical k-mers below that group, a table built
// once per k on the host) plus a ballot prefix.

// (SL_BITS, SL_BINS, SL_NT, SL_SC, SL_LDS_WORDS, SL_WG_PER_CU: vectorise_layout.h)

// even bits of x packed into the low half (inverse of spread_bits, for up to 16 pairs)
__device__ __forceinline__ uint32_t squeeze_bits(uint32_t x)
{
    x &= 0x55555555u;
    x = (x | (x >> 1)) & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    x = (x | (x >> 8)) & 0x0000FFFFu;
    return x;
}

// CGR pixel (i << K) + j of a k-mer index: the inverse of cgr_pixel_to_kmer.  code = jbit << 1 | !(ibit ^ jbit), so
// jbit = high bit of the code, ibit = high ^ low ^ 1; base p (oldest first) is bit p of i and j.
template <int K>
__device__ __forceinline__ uint32_t kmer_to_cgr_pixel(uint32_t b)
{
    constexpr uint32_t M = (1u << K) - 1u;
    const uint32_t hi = squeeze_bits(b >> 1), lo = squeeze_bits(b);   // base p at bit K-1-p
    const uint32_t j = __brev(hi) >> (32 - K);
    const uint32_t i = __brev((hi ^ lo ^ M) & M) >> (32 - K);
    return (i << K) | j;
}

template <int K>
__device__ __forceinline__ uint32_t slice_bin(uint32_t km, int mode)
{
    if (mode == IDL_MODE_CGR) return kmer_to_cgr_pixel<K>(km);
    if (mode == IDL_MODE_CANONICAL) { const uint32_t rc = revcomp<K>(km); return rc < km ? rc : km; }
    return km;
}

// Where the items of a launch come from.  The whole-store kernel takes item `it` of the grid as (sequence it / n_views, view it % n_views) and
// stores the row as the vectoriser made it; vectorise_pairs.h takes the item from a pair list and standardises the float32 row on its way out.
struct SliceGridItems {
    __device__ __forceinline__ int64_t count(const VecArgs &a) const { return a.n * a.n_views; }
    __device__ __forceinline__ bool item(const VecArgs &a, int64_t it, int64_t row_len, int64_t &s, int &v, int64_t &out_base) const
    {
        s = it / a.n_views;
        v = (int)(it - s * a.n_views);
        out_base = (int64_t)v * a.view_stride + s * row_len;
        return true;
    }
    // four float32 frequencies of the row, at a.out + o (col: the row's column of f.x)
    __device__ __forceinline__ void store_f32(const VecArgs &a, int64_t o, int64_t, float4 f) const { *(float4 *)((float *)a.out + o) = f; }
};

// one workgroup's share of the items: the body of vectorise_slices_kernel and of vectorise_pairs_slices_kernel
template <int K, typename Items>
__device__ __forceinline__ void slices_body(const VecArgs &a, const int32_t *rank_tab, const Items &items)
{
    constexpr int F = 1 << (2 * K);
    constexpr uint32_t KM = (1u << (2 * K)) - 1u;
    constexpr int NS = F / SL_BINS;             // slices of the bin space: 4 at k = 8, 16 at k = 9
    constexpr int NW = SL_NT / 64;
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *hist = lds;                       // SL_BINS bins of the current slice, in output order
    uint32_t *cod = lds + SL_BINS;              // (SL_SC + 1) slots x 4 words, slot 0 = halo
    uint32_t *msk = cod + (SL_SC + 1) * 4;      // (SL_SC + 1) slots x 2 words
    int64_t *red = (int64_t *)(msk + (SL_SC + 1) * 2);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    auto block_sum = [&](int64_t v) -> int64_t {
        v = wave_sum_i64(v);
        __syncthreads();
        if (lane == 0) red[wave] = v;
        __syncthreads();
        int64_t t = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) t += red[w];
        return t;
    };
    const bool canonical = a.mode == IDL_MODE_CANONICAL;
    const int64_t row_len = canonical ? ((K % 2 == 0) ? (F + (1 << K)) / 2 : F / 2) : F;
    const uint32_t iv = (a.init == IDL_INIT_ONE) ? 1u : 0u;
    const int first_sweep = (canonical && a.out_kind != IDL_OUT_COUNTS_I32) ? 0 : 1;

    const int64_t n_items = items.count(a);
    for (int64_t it = blockIdx.x; it < n_items; it += gridDim.x) {
        int64_t s, out_base;
        int v;
        if (!items.item(a, it, row_len, s, v, out_base)) continue;      // (the same answer in every thread of the workgroup)
        const int64_t slot0 = a.slot_off[s];
        const int64_t L = a.lengths[s];
        const int64_t nslots = (L + 63) >> 6;
        const int64_t nsc = (nslots + SL_SC - 1) / SL_SC;
        const uint32_t *E = nullptr;
        int64_t ne = 0;
        if (a.edits != nullptr) {
            const int64_t eb = eo_begin(a, (int64_t)v * a.n + s);
            ne = eo_end(a, (int64_t)v * a.n + s) - eb;
            E = a.edits + eb;
            if (ne < 0) ne = 0;
        }

        // global -> LDS: slots [sc * SL_SC - 1, sc * SL_SC + nloc) with this view's edits applied; returns nloc
        auto stage = [&](int64_t sc) -> int {
            const int64_t sc_first = sc * SL_SC;
            const int nloc = (int)((nslots - sc_first) < SL_SC ? (nslots - sc_first) : SL_SC);
            __syncthreads();
            for (int i = tid; i < nloc + 1; i += SL_NT) {
                const int64_t g = sc_first - 1 + i;
                uint4 c = make_uint4(0u, 0u, 0u, 0u);
                uint2 m = make_uint2(0xFFFFFFFFu, 0xFFFFFFFFu);
                if (g >= 0) { c = a.codes[slot0 + g]; m = a.mask[slot0 + g]; }
                *(uint4 *)(cod + i * 4) = c;
                *(uint2 *)(msk + i * 2) = m;
            }
            __syncthreads();
            if (ne > 0) {
                const int64_t lo = (sc_first - 1) * 64, hi = (sc_first + nloc) * 64;   // staged positions [lo, hi)
                int64_t e0 = 0, e1 = ne;                                               // first edit at or after lo (edits are sorted)
                while (e0 < e1) {
                    const int64_t mid = (e0 + e1) >> 1;
                    if ((int64_t)(E[mid] & 0x3FFFFFFFu) < lo) e0 = mid + 1; else e1 = mid;
                }
                for (int64_t e = e0 + tid; e < ne; e += SL_NT) {
                    const uint32_t ed = E[e];
                    const int64_t pos = (int64_t)(ed & 0x3FFFFFFFu);
                    if (pos >= hi) break;
                    const uint32_t rel = (uint32_t)(pos - lo), op = ed >> 30;
                    if (op == 0u) atomicOr(&msk[rel >> 5], 0x80000000u >> (rel & 31u));
                    else atomicXor(&cod[rel >> 4], op << (30u - 2u * (rel & 15u)));
                }
                __syncthreads();
            }
            return nloc;
        };

        int nloc0 = 0;
        if (nsc == 1) nloc0 = stage(0);
        int64_t windows = 0, S = 0;
        bool have_windows = false;

        for (int sweep = first_sweep; sweep < 2; ++sweep) {
            int64_t part = 0;                    // sweep 0: this thread's share of the canonical row's truncated sum
            for (int sl = 0; sl < NS; ++sl) {
                const uint32_t lo_bin = (uint32_t)sl * SL_BINS;

                // ---------------- the slice's starting counts
                __syncthreads();
                if (a.init == IDL_INIT_FROM_OUT) {
                    const uint4 *src = (const uint4 *)((const uint32_t *)a.out + out_base + lo_bin);
                    for (int i = tid; i < SL_BINS / 4; i += SL_NT) *(uint4 *)(hist + i * 4) = src[i];
                } else if (canonical && iv != 0u) {
                    // a canonical bin holds both strands' pseudocounts; a palindrome (even k only) is its own partner
                    for (int i = tid; i < SL_BINS; i += SL_NT) {
                        const uint32_t b = lo_bin + i;
                        hist[i] = (revcomp<K>(b) == b) ? 1u : 2u;
                    }
                } else {
                    for (int i = tid; i < SL_BINS / 4; i += SL_NT) *(uint4 *)(hist + i * 4) = make_uint4(iv, iv, iv, iv);
                }
                __syncthreads();

                // ---------------- one walk over the windows: count those whose output bin lies in [lo_bin, lo_bin + SL_BINS)
                uint32_t cnt = 0;
                for (int64_t sc = 0; sc < nsc; ++sc) {
                    const int nloc = (nsc == 1) ? nloc0 : stage(sc);
                    const int nd = nloc * 4;
                    for (int d = tid; d < nd; d += SL_NT) {
                        const int D = 4 + d;
                        const uint64_t w = ((uint64_t)cod[D - 1] << 32) | cod[D];
                        const uint32_t m0 = msk[(D >> 1) - 1], m1 = msk[D >> 1];
                        const uint32_t M = (D & 1) ? m1 : (uint32_t)((((uint64_t)m0 << 32) | m1) >> 16);
                        uint32_t inv = M;
#pragma unroll
                        for (int t = 1; t < K; ++t) inv |= (M >> t);
                        inv &= 0xFFFFu;
#pragma unroll
                        for (int j = 0; j < 16; ++j) {
                            const uint32_t bin = slice_bin<K>((uint32_t)(w >> (30 - 2 * j)) & KM, a.mode) - lo_bin;
                            if (bin < (uint32_t)SL_BINS && !((inv >> (15 - j)) & 1u)) atomicAdd(&hist[bin], 1u);
                        }
                        cnt += 16u - (uint32_t)__popc(inv);
                    }
                }
                if (!have_windows) {             // the number of valid windows does not depend on the slice
                    windows = block_sum((int64_t)cnt);
                    have_windows = true;
                }
                __syncthreads();

                // ---------------- epilogue of the slice
                if (canonical) {
                    for (int g = wave; g < SL_BINS / 64; g += NW) {
                        const uint32_t i = (uint32_t)g * 64 + lane, b = lo_bin + i;
                        const uint32_t rc = revcomp<K>(b);
                        const bool canon = b <= rc;
                        const int32_t val = canon ? (int32_t)(b == rc ? hist[i] : hist[i] / 2u) : 0;
                        if (sweep == 0) { part += val; continue; }
                        const uint64_t bal = __ballot(canon);
                        if (canon) {
                            const int64_t o = out_base + rank_tab[(lo_bin >> 6) + g] + __popcll(bal & ((1ull << lane) - 1ull));
                            if (a.out_kind == IDL_OUT_COUNTS_I32) ((int32_t *)a.out)[o] = val;
                            else if (a.out_kind == IDL_OUT_FREQ_F64) ((double *)a.out)[o] = (double)val / (double)S;
                            else ((float *)a.out)[o] = (float)((double)val / (double)S);
                        }
                    }
                } else {
                    // row sum: every bin started at `init` (or at the caller's value) and got `windows` increments
                    const int64_t T = (a.init == IDL_INIT_FROM_OUT) ? 0 : windows + (iv ? (int64_t)F : 0);
                    const bool small = T < (1ll << 24);  // then int -> float32 is exact and f32 division == f64 division rounded
                    const float Sf = (float)T;
                    const double Sd = (double)T;
                    for (int i4 = tid; i4 < SL_BINS / 4; i4 += SL_NT) {
                        const uint4 h = *(const uint4 *)(hist + i4 * 4);
                        const int64_t o = out_base + lo_bin + i4 * 4;
                        if (a.out_kind == IDL_OUT_COUNTS_I32) {
                            *(uint4 *)((uint32_t *)a.out + o) = h;
                        } else if (a.out_kind == IDL_OUT_FREQ_F64) {
                            double *dst = (double *)a.out + o;
                            *(double2 *)dst = make_double2((double)h.x / Sd, (double)h.y / Sd);
                            *(double2 *)(dst + 2) = make_double2((double)h.z / Sd, (double)h.w / Sd);
                        } else {
                            float4 f;
                            if (small) {
                                f.x = (float)h.x / Sf; f.y = (float)h.y / Sf;
                                f.z = (float)h.z / Sf; f.w = (float)h.w / Sf;
                            } else {
                                f.x = (float)((double)h.x / Sd); f.y = (float)((double)h.y / Sd);
                                f.z = (float)((double)h.z / Sd); f.w = (float)((double)h.w / Sd);
                            }
                            items.store_f32(a, o, (int64_t)lo_bin + i4 * 4, f);
                        }
                    }
                }
            }
            if (sweep == 0) S = block_sum(part);
        }
        __syncthreads();
    }
}

template <int K>
__global__ __launch_bounds__(SL_NT) void vectorise_slices_kernel(VecArgs a, const int32_t *rank_tab)
{
    slices_body<K>(a, rank_tab, SliceGridItems{});
}

// rank_tab[g] = canonical k-mers (b <= rc(b)) below bin 64 * g, g in [0, 4^k / 64]; built on the host once per (device, k)
template <int K>
const int32_t *slices_rank_table()
{
    static std::mutex mu;
    static std::map<int, int32_t *> tabs;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return nullptr;
    std::lock_guard<std::mutex> lock(mu);
    int32_t *&p = tabs[dev];
    if (p != nullptr) return p;
    constexpr uint32_t F = 1u << (2 * K);
    std::vector<int32_t> h(F / 64 + 1);
    int32_t rank = 0;
    for (uint32_t b = 0; b < F; ++b) {
        if ((b & 63u) == 0u) h[b >> 6] = rank;
        uint32_t rc = 0, x = ~b;
        for (int t = 0; t < K; ++t) { rc = (rc << 2) | (x & 3u); x >>= 2; }
        if (b <= rc) ++rank;
    }
    h[F / 64] = rank;
    if (hipMalloc((void **)&p, h.size() * sizeof(int32_t)) != hipSuccess) { p = nullptr; return nullptr; }
    if (hipMemcpy(p, h.data(), h.size() * sizeof(int32_t), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(p);
        p = nullptr;
    }
    return p;
}
