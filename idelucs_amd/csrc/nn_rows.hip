// nn_rows.hip -- idl_nn_rows: for every row of a query set q [m, 64] its exact nearest row of a corpus x [n, 64] (FittedEnsemble.assign
// in the fine-grained mode: a new sequence takes the label of the nearest training latent; and, with self-exclusion, every training point's
// spacing).  m x n pairs in 64 dimensions, nothing of size m x n written.
//
// The distance is idl_knn_select's: float64 from the difference vector, t = (double)q_c - (double)x_c, acc += t * t with c ascending,
// product and sum each rounded -- a query that is a copy of a corpus row is at distance exactly 0 from it, which the float32 Gram form
// |q|^2 + |x|^2 - 2 q.x does not give.  The answer is the j that minimises (D, j) lexicographically, so it is a function of q and x alone:
//
//   nn_rows_kernel   a workgroup holds 256 queries, one per lane, widened to float64 in registers (128 VGPRs); its slice of the corpus goes
//                    through LDS 64 rows at a time, widened once when staged (32 KB).  Every lane reads the same row -- an LDS broadcast,
//                    no bank conflict -- and spends three float64 VALU operations per coordinate (subtract, multiply, add); a lane scans
//                    j ascending and replaces its best only by a strictly smaller D, which is the order.
//                    (Measured at 10^5 x 10^6 and not adopted, same results: two queries a lane on 128 threads, so that one LDS read serves
//                    both -- 256 VGPRs + 78 AGPRs, one wave a SIMD, 1665 ms against 850; the corpus widened into a workspace and read through
//                    scalar loads, no LDS and no barrier -- 1820 ms.  DESIGN.md section 9.)
//   nn_merge_kernel  few queries leave most of the device idle, so the corpus is then cut into slices over blockIdx.y (whole 64-row
//                    chunks; nn_slices: a function of m and n only); every slice leaves its (D, j) per query in a workspace and this launch
//                    takes their minimum by the same order.  Integer comparisons of exact values: no float atomics, no dependence on
//                    which workgroup finished first.
#include "common.h"
#include "wave_ops.h"

namespace {

constexpr int KD = 64;                // point dimension (the latent width of NetLinear / myNet)
constexpr int NQ = 256;               // queries of a workgroup, one per lane
constexpr int NCH = 64;               // corpus rows of one LDS chunk (float64: 32 KB)
constexpr int TARGET_WGS = 1024;      // workgroups the slicing aims at: four per compute unit of an MI355X
constexpr int64_t SLICE_MIN_ROWS = 1024;   // a slice is worth a workgroup from here on
constexpr int MAX_SLICES = 64;
constexpr int32_t NO_ROW = 0x7fffffff;

struct NnArgs {
    const float *q, *x;
    int64_t m, n, self0, slice_rows;
    int32_t *idx; double *d2;         // [m]: the results (one slice) ...
    int32_t *part_idx; double *part_d2;   // ... or [slices, m]: every slice's own (NULL for one slice)
};

__global__ __launch_bounds__(NQ) void nn_rows_kernel(NnArgs a)
{
    __shared__ double xs[NCH * KD];
    const int tid = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * NQ + tid;
    const bool live = i < a.m;
    double qv[KD];
    {   // (a lane past m scans a copy of the last query and writes nothing)
        const float4 *qr = (const float4 *)(a.q + (live ? i : a.m - 1) * KD);
#pragma unroll
        for (int c = 0; c < KD / 4; ++c) {
            const float4 v = qr[c];
            qv[4 * c] = (double)v.x; qv[4 * c + 1] = (double)v.y; qv[4 * c + 2] = (double)v.z; qv[4 * c + 3] = (double)v.w;
        }
    }
    const int64_t j0 = (int64_t)blockIdx.y * a.slice_rows;
    const int64_t j1 = j0 + a.slice_rows < a.n ? j0 + a.slice_rows : a.n;
    const int64_t skip = a.self0 >= 0 ? a.self0 + i : -1;
    double best = __longlong_as_double(0x7ff0000000000000ll);       // +inf: a D that is not below it (inf, NaN) is no neighbour
    int32_t best_j = NO_ROW;
    for (int64_t c0 = j0; c0 < j1; c0 += NCH) {
        const int rows = (int)(j1 - c0 < NCH ? j1 - c0 : NCH);
        __syncthreads();                                            // the previous chunk has been read by every lane
        const float4 *src = (const float4 *)(a.x + c0 * KD);
#pragma unroll
        for (int u = 0; u < NCH * KD / 4 / NQ; ++u) {
            const int e = tid + NQ * u;                             // float4 e of the chunk: row e / 16
            if (e < rows * (KD / 4)) {
                const float4 v = src[e];
                xs[4 * e] = (double)v.x; xs[4 * e + 1] = (double)v.y; xs[4 * e + 2] = (double)v.z; xs[4 * e + 3] = (double)v.w;
            }
        }
        __syncthreads();
#pragma unroll 2
        for (int r = 0; r < rows; ++r) {
            const double *xr = xs + r * KD;
            double d = 0.0;
#pragma unroll
            for (int c = 0; c < KD; ++c) d = idl_dev::square_then_add(d, qv[c] - xr[c]);
            const int64_t j = c0 + r;
            if (d < best && j != skip) { best = d; best_j = (int32_t)j; }     // j ascends: a tie keeps the lower index
        }
    }
    if (!live) return;
    if (a.part_idx != nullptr) {
        a.part_idx[(int64_t)blockIdx.y * a.m + i] = best_j;
        a.part_d2[(int64_t)blockIdx.y * a.m + i] = best;
    } else {
        a.idx[i] = best_j == NO_ROW ? -1 : best_j;
        a.d2[i] = best;
    }
}

__global__ __launch_bounds__(256) void nn_merge_kernel(const int32_t *part_idx, const double *part_d2, int slices, int64_t m, int32_t *idx, double *d2)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= m) return;
    double best = part_d2[i];
    int32_t best_j = part_idx[i];
    for (int s = 1; s < slices; ++s) {
        const double d = part_d2[(int64_t)s * m + i];
        const int32_t j = part_idx[(int64_t)s * m + i];
        if (d < best || (d == best && j < best_j)) { best = d; best_j = j; }
    }
    idx[i] = best_j == NO_ROW ? -1 : best_j;
    d2[i] = best;
}

// (slices, rows of a slice) for m queries against n corpus rows: a function of the two sizes alone
inline int nn_slices(int64_t m, int64_t n, int64_t *slice_rows)
{
    const int64_t tiles = (m + NQ - 1) / NQ;
    int64_t s = tiles > 0 ? (TARGET_WGS + tiles - 1) / tiles : 1;
    if (s > n / SLICE_MIN_ROWS) s = n / SLICE_MIN_ROWS;
    if (s > MAX_SLICES) s = MAX_SLICES;
    if (s < 1) s = 1;
    const int64_t rows = ((n + s - 1) / s + NCH - 1) / NCH * NCH;   // whole chunks; the last slice takes what is left
    if (slice_rows) *slice_rows = rows;
    return (int)((n + rows - 1) / rows);
}

}  // namespace

extern "C" {

int idl_nn_rows_slices(int64_t m, int64_t n)
{
    IDL_REQUIRE(m >= 0 && n >= 1 && n < (1ll << 31), "nn_rows_slices: bad sizes");
    return nn_slices(m, n, nullptr);
}

int idl_nn_rows(const float *q, int64_t m, const float *x, int64_t n, int d, int64_t self0, int32_t *idx, double *d2, void *stream)
{
    IDL_REQUIRE(d == KD, "nn_rows: points must have 64 coordinates");
    IDL_REQUIRE(n >= 1 && n < (1ll << 31) && m >= 0 && (m + NQ - 1) / NQ < (1ll << 31), "nn_rows: bad sizes (1 <= n < 2^31, m >= 0)");
    IDL_REQUIRE(self0 < 0 || n >= 2, "nn_rows: self-exclusion needs a corpus of at least two rows");
    if (m == 0) return IDL_OK;
    IDL_REQUIRE(q && x && idx && d2, "nn_rows: NULL buffer");
    IDL_REQUIRE(((((uintptr_t)q) | ((uintptr_t)x)) & 15u) == 0, "nn_rows: q and x must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    NnArgs a{q, x, m, n, self0, 0, idx, d2, nullptr, nullptr};
    const int slices = nn_slices(m, n, &a.slice_rows);
    const unsigned tiles = (unsigned)((m + NQ - 1) / NQ);
    if (slices == 1) {
        hipLaunchKernelGGL(nn_rows_kernel, dim3(tiles, 1), dim3(NQ), 0, st, a);
        IDL_HIP_TRY(hipGetLastError());
        return IDL_OK;
    }
    // the slices' partial results: 12 bytes per (slice, query), allocated and freed in stream order
    void *ws = nullptr;
    const size_t cells = (size_t)slices * (size_t)m;
    IDL_HIP_TRY(hipMallocAsync(&ws, cells * 12, st));
    a.part_d2 = (double *)ws;
    a.part_idx = (int32_t *)((unsigned char *)ws + cells * 8);
    hipLaunchKernelGGL(nn_rows_kernel, dim3(tiles, (unsigned)slices), dim3(NQ), 0, st, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
        hipLaunchKernelGGL(nn_merge_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, a.part_idx, a.part_d2, slices, m, idx, d2);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(ws, st);
    IDL_HIP_TRY(e);
    return IDL_OK;
}

}  // extern "C"
