// embed.hip -- the 2-D picture of the latent that --plot saves (reference idelucs/__main__.py:239-247: umap.UMAP(random_state=42)
// .fit_transform(latent), scattered into learned_representation.jpg).  The `umap` package is absent; this is UMAP's algorithm on
// the device, in three stages (posthoc.umap_embedding_device drives them; DESIGN.md section 7 has the derivation):
//
//   exact kNN graph        posthoc.knn_graph_device: idl_knn_window's pass with idl_knn_graph (knn.hip) behind it;
//   idl_umap_smooth_knn    per row, in double: rho = the smallest positive distance, sigma = the root of
//                          sum_j exp(-max(0, d_ij - rho) / sigma) = log2(k) by UMAP's bisection -- ALWAYS 64 rounds, which pins
//                          the root to double precision (umap-learn stops at 1e-5) -- the floor, and the directed weights.
//                          The fuzzy union P = A + A^T - A o A^T and the pruning are torch sort / unique plumbing on the device;
//   idl_umap_layout_epoch  one launch per epoch of optimize_layout_euclidean as a JACOBI sweep: every force is computed from the
//                          positions at the start of the epoch (one buffer), the result goes to the other; a lane group owns a
//                          vertex and walks its CSR row.  No atomics: the sum of a vertex is taken in a fixed order -- a lane's
//                          entries in CSR order, per entry the attraction then its draws, then a butterfly across the lanes --
//                          so the same inputs give the same bits on every run, which hogwild SGD does not.
//
// Draw scheme (tests/umap_ref.py restates it): Philox4x32-10 (philox_device.h) with key (seed low, seed high) and counter
// (entry index low, entry index high, epoch, draw group); draw p of an entry in an epoch is word p % 4 (x, y, z, w) of group p / 4,
// and the vertex it names is mulhi(word, N) = (word * N) >> 32.  The entry index is the position of the directed entry in the CSR.
// The start's jitter (idl_umap_jitter) uses counter (vertex low, vertex high, 0, 0xffffffff): coordinate c gets
// scale * (2 u - 1), u = (word c >> 8) * 2^-24.
#include "common.h"
#include "philox_device.h"

namespace {

constexpr int LG = 8;             // lanes that own a vertex (why 8 and not 16)

__device__ __forceinline__ uint32_t word_of(const idl_dev::U4 &r, int w)
{
    return w == 0 ? r.x : w == 1 ? r.y : w == 2 ? r.z : r.w;
}

// the draw scheme, in one place: the Philox group g of (entry, epoch), and the vertex that word p % 4 of group p / 4 names
__device__ __forceinline__ idl_dev::U4 draw_group(int64_t e, int epoch, int64_t g, uint32_t k0, uint32_t k1)
{
    return idl_dev::philox((uint32_t)e, (uint32_t)((uint64_t)e >> 32), (uint32_t)epoch, (uint32_t)g, k0, k1);
}
__device__ __forceinline__ int64_t drawn_vertex(const idl_dev::U4 &r, int64_t p, int64_t n)
{
    return (int64_t)(((uint64_t)word_of(r, (int)(p & 3)) * (uint64_t)n) >> 32);
}

__device__ __forceinline__ float clip4(float v) { return fminf(fmaxf(v, -4.f), 4.f); }

struct SmoothArgs {
    const double *dist;           // [n, k] ascending, the point itself included
    const int32_t *idx;           // [n, k]
    int64_t n; int k;
    double mean_all;              // mean of all n * k distances
    double *rho, *sigma;          // [n]
    double *w;                    // [n, k] directed weights
};

__global__ __launch_bounds__(256) void umap_smooth_knn_kernel(SmoothArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= a.n) return;
    const double *d = a.dist + i * a.k;
    double rho = 0.0, sum = 0.0;
    bool any = false;
    for (int j = 0; j < a.k; ++j) {
        const double v = d[j];
        sum += v;
        if (v > 0.0 && (!any || v < rho)) { rho = v; any = true; }
    }
    const double target = log2((double)a.k);
    double lo = 0.0, hi = INFINITY, mid = 1.0;
    for (int round = 0; round < 64; ++round) {
        double psum = 0.0;
        for (int j = 1; j < a.k; ++j) psum += exp(-fmax(0.0, d[j] - rho) / mid);
        if (psum > target) { hi = mid; mid = (lo + hi) / 2.0; }
        else { lo = mid; mid = hi == INFINITY ? mid * 2.0 : (lo + hi) / 2.0; }
    }
    const double floor_ = 1e-3 * (rho > 0.0 ? sum / (double)a.k : a.mean_all);
    const double sigma = mid < floor_ ? floor_ : mid;
    a.rho[i] = rho; a.sigma[i] = sigma;
    for (int j = 0; j < a.k; ++j)
        a.w[i * a.k + j] = a.idx[i * a.k + j] == i ? 0.0 : exp(-fmax(0.0, d[j] - rho) / sigma);
}

struct LayoutArgs {
    const float2 *y_in; float2 *y_out;
    int64_t n;
    const int64_t *indptr;        // [n + 1]
    const int32_t *indices;       // [entries]
    const double *eps;            // [entries] epochs per sample = max(P) / P_e
    double *next, *next_neg;      // [entries] schedule state, touched by the row's owner only
    int epoch;                    // 1 ..
    float alpha, ca, cb;          // learning rate of this epoch; the curve constants a, b
    uint32_t k0, k1;              // the seed
};

__global__ __launch_bounds__(256) void umap_layout_epoch_kernel(LayoutArgs a)
{
#pragma clang fp contract(off)        // products and sums each rounded, as the float32 replay of tests/umap_ref.py takes them
    const int64_t v = ((int64_t)blockIdx.x * 256 + threadIdx.x) / LG;
    const int lane = threadIdx.x & (LG - 1);
    const bool ok = v < a.n;                       // the same for the LG lanes of a vertex (LG divides 256)
    float sx = 0.f, sy = 0.f;
    float2 yj = float2{0.f, 0.f};
    if (ok) {
        yj = a.y_in[v];
        const double ep = (double)a.epoch;
        const int64_t e1 = a.indptr[v + 1];
        for (int64_t e = a.indptr[v] + lane; e < e1; e += LG) {
            const double nx = a.next[e];
            if (!(nx <= ep)) continue;
            const double es = a.eps[e], esn = es / 5.0, nn = a.next_neg[e];
            {   // attraction, counted twice: entry (k, j) fires in the same epochs and moves its tail j by the same amount
                const float2 yk = a.y_in[a.indices[e]];
                const float dx = yj.x - yk.x, dy = yj.y - yk.y, d2 = dx * dx + dy * dy;
                float c = 0.f;
                if (d2 > 0.f) { const float pb = powf(d2, a.cb); c = (-2.f * a.ca * a.cb * (pb / d2)) / (a.ca * pb + 1.f); }
                sx += 2.f * clip4(c * dx); sy += 2.f * clip4(c * dy);
            }
            const int64_t n_neg = (int64_t)floor((ep - nn) / esn);
            idl_dev::U4 r{0, 0, 0, 0};
            for (int64_t p = 0; p < n_neg; ++p) {
                if ((p & 3) == 0) r = draw_group(e, a.epoch, p >> 2, a.k0, a.k1);
                const int64_t s = drawn_vertex(r, p, a.n);
                if (s == v) continue;
                const float2 ys = a.y_in[s];
                const float dx = yj.x - ys.x, dy = yj.y - ys.y, d2 = dx * dx + dy * dy;
                if (d2 > 0.f) {
                    const float pb = powf(d2, a.cb);
                    const float c = (2.f * a.cb) / ((0.001f + d2) * (a.ca * pb + 1.f));
                    sx += clip4(c * dx); sy += clip4(c * dy);
                } else { sx += 4.f; sy += 4.f; }
            }
            a.next[e] = nx + es;
            a.next_neg[e] = nn + (double)n_neg * esn;
        }
    }
    // fixed butterfly over the LG lanes of the vertex: every lane ends with the same sum
#pragma unroll
    for (int o = 1; o < LG; o <<= 1) { sx += __shfl_xor(sx, o, LG); sy += __shfl_xor(sy, o, LG); }
    if (ok && lane == 0) a.y_out[v] = float2{yj.x + a.alpha * sx, yj.y + a.alpha * sy};
}

__global__ __launch_bounds__(256) void umap_draws_kernel(int64_t e0, int64_t count, int epoch, int n_draws, int64_t n, uint32_t k0, uint32_t k1, int32_t *out)
{
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= count * n_draws) return;
    const int64_t e = e0 + t / n_draws;
    const int p = (int)(t % n_draws);
    out[t] = (int32_t)drawn_vertex(draw_group(e, epoch, p >> 2, k0, k1), p, n);
}

__global__ __launch_bounds__(256) void umap_jitter_kernel(float2 *y, int64_t n, float scale, uint32_t k0, uint32_t k1)
{
#pragma clang fp contract(off)        // y + scale * (2 u - 1) with every product and sum rounded, as tests/umap_ref.py's jitter
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= n) return;
    const idl_dev::U4 r = idl_dev::philox((uint32_t)v, (uint32_t)((uint64_t)v >> 32), 0u, 0xffffffffu, k0, k1);
    float2 p = y[v];
    p.x += scale * (2.f * ((float)(r.x >> 8) * 5.9604645e-8f) - 1.f);
    p.y += scale * (2.f * ((float)(r.y >> 8) * 5.9604645e-8f) - 1.f);
    y[v] = p;
}

}  // namespace

extern "C" {

int idl_umap_smooth_knn(const double *dist, const int32_t *idx, int64_t n, int k, double mean_all, double *rho, double *sigma, double *w, void *stream)
{
    IDL_REQUIRE(dist && idx && rho && sigma && w, "umap_smooth_knn: NULL buffer");
    IDL_REQUIRE(n >= 1 && n < (1ll << 31) && k >= 2 && k <= n, "umap_smooth_knn: needs 2 <= k <= n < 2^31");
    SmoothArgs a{dist, idx, n, k, mean_all, rho, sigma, w};
    hipLaunchKernelGGL(umap_smooth_knn_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

int idl_umap_layout_epoch(const float *y_in, float *y_out, int64_t n, const int64_t *indptr, const int32_t *indices, const double *eps,
                          double *next, double *next_neg, int epoch, float alpha, float a, float b, uint64_t seed, void *stream)
{
    IDL_REQUIRE(y_in && y_out && indptr && y_in != y_out, "umap_layout_epoch: NULL buffer, or one buffer for both sides of the sweep");
    IDL_REQUIRE(n >= 1 && n < (1ll << 28) && epoch >= 1, "umap_layout_epoch: needs 1 <= n < 2^28 and epoch >= 1");
    IDL_REQUIRE((((uintptr_t)y_in | (uintptr_t)y_out) & 7u) == 0, "umap_layout_epoch: positions must be 8-byte aligned");
    LayoutArgs args{(const float2 *)y_in, (float2 *)y_out, n, indptr, indices, eps, next, next_neg, epoch, alpha, a, b,
                    (uint32_t)seed, (uint32_t)(seed >> 32)};
    hipLaunchKernelGGL(umap_layout_epoch_kernel, dim3((unsigned)((n * LG + 255) / 256)), dim3(256), 0, (hipStream_t)stream, args);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

int idl_umap_draws(uint64_t seed, int64_t entry0, int64_t count, int epoch, int n_draws, int64_t n, int32_t *out, void *stream)
{
    IDL_REQUIRE(out && count >= 1 && n_draws >= 1 && count * n_draws < (1ll << 31) && n >= 1 && n < (1ll << 31) && entry0 >= 0, "umap_draws: bad sizes");
    hipLaunchKernelGGL(umap_draws_kernel, dim3((unsigned)((count * n_draws + 255) / 256)), dim3(256), 0, (hipStream_t)stream, entry0, count, epoch,
                       n_draws, n, (uint32_t)seed, (uint32_t)(seed >> 32), out);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

int idl_umap_jitter(float *y, int64_t n, float scale, uint64_t seed, void *stream)
{
    IDL_REQUIRE(y && n >= 1 && n < (1ll << 31) && (((uintptr_t)y) & 7u) == 0, "umap_jitter: bad buffer or size");
    hipLaunchKernelGGL(umap_jitter_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (float2 *)y, n, scale,
                       (uint32_t)seed, (uint32_t)(seed >> 32));
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

}  // extern "C"
