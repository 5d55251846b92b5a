// small_predict.hip -- the eval forward of model_size='small' (myNet, reference idelucs/PytorchUtils.py:6-31) on this library's own launches: what
// IID_model.predict / calculate_probs / predict_latent_shard and a saved ensemble's assign run when they are asked for small_predict='native'
// (idelucs_amd/predict_native.py: NativeSmallPredictor).
//
//   idl_small_predict_l1   a1 [m, 400] = x W1^T                      Linear(F', 400) of PytorchUtils.py:13 without its bias, shaped for predict's tall blocks
//   idl_small_predict_mid  r1 = ReLU(a1 + b1); a2 = LeakyReLU_0.01(r1 W2^T + b2); lat = a2 Wi^T + bi; z = softmax(a2 Wc^T + bc); prob = max z; unit = its
//                          lowest class                              PytorchUtils.py:15-22 in eval mode (both Dropouts are the identity), as called at models.py:158-170
//
// A row's outputs are a function of that row and of the weights alone.  Row l of a 16 x 16 MFMA tile takes its A operand from lane l's registers only, every
// output element has ONE accumulator to which its K is added in the same order whatever m, the tile or the block (layer 1: the 32-wide stages in ascending
// order, a function of F' alone; the middle launch: fixed), the per-row stages run one row a wave, and there are no atomics.
// Rows past m in the last tile are computed (layer 1: on row m - 1's entries; the middle launch: on zeros) and not stored.
#include "common.h"
#include "mid_fwd_device.h"

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int SH1 = 400;          // myNet's hidden widths
constexpr int SH2 = 128;
constexpr int SLAT = 64;          // latent (instance head)
constexpr int SMAX_C = 64 * mid_dev::MAX_CPL;
constexpr float SLOPE = 0.01f;    // nn.LeakyReLU() default

__device__ __forceinline__ f32x4_t mfma(float a, float b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// ---------------------------------------------------------------- layer 1: a1[m, 400] = x W1^T, 128 rows x 400 units a workgroup of 8 waves
// A stage is 32 consecutive k of the workgroup's 128 rows of x and of all 400 rows of W1, staged in LDS once ([528][32 + 4] floats) and read by every wave:
// wave w owns rows 16 w .. 16 w + 15 and all 25 column tiles (25 accumulators); lane group q holds the four consecutive k 16 h + 4q .. + 3 of half h of the
// stage (one ds_read_b128 of x and of each W1 row for four MFMAs), five column tiles interleaved so that an accumulator's next MFMA is five issues away.
// Two stage buffers: the next stage's global reads are issued before this stage's MFMAs and written to the other buffer behind them; one barrier a stage.
// A float4 at or beyond F' (F' % 4 == 0) is staged as zeros: the tail stage adds +0 products.
constexpr int P1_WAVES = 8, P1_THREADS = 64 * P1_WAVES, P1_ROWS = 16 * P1_WAVES, P1_KC = 32, P1_LD = P1_KC + 4;
constexpr int P1_SROWS = P1_ROWS + SH1;                                 // 528 staged rows: x, then W1
constexpr int P1_LOADS = (P1_SROWS * (P1_KC / 4) + P1_THREADS - 1) / P1_THREADS;       // float4s a thread stages: 9 (the last one: threads 0..127)
constexpr int P1_CT = SH1 / 16, P1_CG = 5;                              // 25 column tiles, in groups of 5
constexpr int P1_LDS_BYTES = 2 * P1_SROWS * P1_LD * 4;                  // 152 064
static_assert(P1_CT % P1_CG == 0 && P1_THREADS / (P1_KC / 4) == 64, "layer-1 predict tile");

__global__ __launch_bounds__(P1_THREADS) void small_predict_l1_kernel(const float *__restrict__ x, const float *__restrict__ W1, int m, int F,
                                                                      float *__restrict__ a1)
{
    extern __shared__ __attribute__((aligned(16))) float p1_lds[];
    float (*S)[P1_SROWS][P1_LD] = (float (*)[P1_SROWS][P1_LD])p1_lds;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l = lane & 15, q = lane >> 4;
    const int r0 = (int)blockIdx.x * P1_ROWS;
    // this thread's staged float4s: column 4 (tid & 7) of staged rows (tid >> 3) + 64 i
    const int sc = 4 * (tid & 7), sr = tid >> 3;
    const float *src[P1_LOADS];
#pragma unroll
    for (int i = 0; i < P1_LOADS; ++i) {
        const int row = sr + 64 * i;                                    // (i == P1_LOADS - 1: rows 512 .. 575, the first 16 of them staged)
        src[i] = row < P1_ROWS ? x + (int64_t)min(r0 + row, m - 1) * F + sc : W1 + (int64_t)min(row - P1_ROWS, SH1 - 1) * F + sc;
    }
    const bool last_on = sr < P1_SROWS - 64 * (P1_LOADS - 1);
    float4 st[P1_LOADS];
    auto fetch = [&](int c) {
        const bool in = P1_KC * c + sc < F;
#pragma unroll
        for (int i = 0; i < P1_LOADS; ++i) {
            st[i] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (in && (i < P1_LOADS - 1 || last_on)) st[i] = *(const float4 *)(src[i] + P1_KC * c);
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int i = 0; i < P1_LOADS; ++i)
            if (i < P1_LOADS - 1 || last_on) *(float4 *)&S[buf][sr + 64 * i][sc] = st[i];
    };
    f32x4_t acc[P1_CT];
#pragma unroll
    for (int ct = 0; ct < P1_CT; ++ct) acc[ct] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const bool live = r0 + 16 * wv < m;                                 // (a wave whose 16 rows are all past m stages and waits, nothing else)
    const int nst = (F + P1_KC - 1) / P1_KC;
    fetch(0);
    stage(0);
    __syncthreads();
    for (int c = 0; c < nst; ++c) {
        const int buf = c & 1;
        if (c + 1 < nst) fetch(c + 1);
        if (live) {
#pragma unroll
            for (int h = 0; h < P1_KC / 16; ++h) {
                const int k = 16 * h + 4 * q;
                const float4 av = *(const float4 *)&S[buf][16 * wv + l][k];
#pragma unroll
                for (int g = 0; g < P1_CT; g += P1_CG) {
                    float4 bv[P1_CG];
#pragma unroll
                    for (int t = 0; t < P1_CG; ++t) bv[t] = *(const float4 *)&S[buf][P1_ROWS + 16 * (g + t) + l][k];
#pragma unroll
                    for (int t = 0; t < P1_CG; ++t) acc[g + t] = mfma(av.x, bv[t].x, acc[g + t]);
#pragma unroll
                    for (int t = 0; t < P1_CG; ++t) acc[g + t] = mfma(av.y, bv[t].y, acc[g + t]);
#pragma unroll
                    for (int t = 0; t < P1_CG; ++t) acc[g + t] = mfma(av.z, bv[t].z, acc[g + t]);
#pragma unroll
                    for (int t = 0; t < P1_CG; ++t) acc[g + t] = mfma(av.w, bv[t].w, acc[g + t]);
                }
            }
        }
        if (c + 1 < nst) stage(buf ^ 1);
        __syncthreads();
    }
    if (!live) return;
#pragma unroll
    for (int ct = 0; ct < P1_CT; ++ct)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = r0 + 16 * wv + 4 * q + r;                     // C/D: row 4q + r, column l
            if (i < m) a1[(int64_t)i * SH1 + 16 * ct + l] = acc[ct][r];
        }
}

// ---------------------------------------------------------------- the middle launch: 16 rows a workgroup of 4 waves
// The stages of small_step.hip's small_mid_fwd_kernel with train = 0, on the same tiles and in the same order; a1 is only read, nothing of a2 / d2 / f / inv
// is stored, there is no Philox draw, the latent leaves raw and the row's largest z and its class leave with it (mid_fwd_device.h's row stage).
struct SmallPredictArgs {
    const float *a1, *b1, *W2, *b2, *Wi, *bi, *Wc, *bc;
    int m, C;
    float *lat, *z, *prob; int32_t *unit;
};

__global__ __launch_bounds__(256) void small_predict_mid_kernel(SmallPredictArgs a)
{
    __shared__ float A1[16][SH1 + 4];
    __shared__ float A2[16][SH2 + 4];
    __shared__ float HL[16][SMAX_C + 4];       // the latent, then the logits
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l = lane & 15, q = lane >> 4;
    const int r0 = (int)blockIdx.x * 16, m = a.m, C = a.C;
    // ---- r1 = ReLU(a1 + b1) (rows past m: zeros)
    for (int e = tid; e < 16 * (SH1 / 4); e += 256) {
        const int rr = e / (SH1 / 4), c = 4 * (e % (SH1 / 4));
        const int64_t row = r0 + rr;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < m) {
            v = *(const float4 *)(a.a1 + row * SH1 + c);
            const float4 bb = *(const float4 *)(a.b1 + c);
            v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w;
            v.x = v.x > 0.f ? v.x : 0.f; v.y = v.y > 0.f ? v.y : 0.f;
            v.z = v.z > 0.f ? v.z : 0.f; v.w = v.w > 0.f ? v.w : 0.f;
        }
        *(float4 *)&A1[rr][c] = v;
    }
    __syncthreads();
    // ---- a2 = LeakyReLU(r1 W2^T + b2): wave wv owns column tiles 2 wv, 2 wv + 1; lane group q holds k = 16 c + 4q .. + 3
    for (int t = 0; t < 2; ++t) {
        const int c0 = 16 * (2 * wv + t);
        const float *wr = a.W2 + (int64_t)(c0 + l) * SH1;
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 5
        for (int c = 0; c < SH1 / 16; ++c) {
            const int k = 16 * c + 4 * q;
            const float4 av = *(const float4 *)&A1[l][k];
            const float4 bv = *(const float4 *)(wr + k);
            acc = mfma(av.x, bv.x, acc); acc = mfma(av.y, bv.y, acc); acc = mfma(av.z, bv.z, acc); acc = mfma(av.w, bv.w, acc);
        }
        const int col = c0 + l;
        const float bb = a.b2[col];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const float v = acc[r] + bb;
            A2[4 * q + r][col] = v > 0.f ? v : SLOPE * v;
        }
    }
    __syncthreads();
    // ---- lat = a2 Wi^T + bi: wave wv owns latent columns 16 wv .. 16 wv + 15
    {
        const int c0 = 16 * wv;
        const float *wr = a.Wi + (int64_t)(c0 + l) * SH2;
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < SH2 / 16; ++c) {
            const int k = 16 * c + 4 * q;
            const float4 av = *(const float4 *)&A2[l][k];
            const float4 bv = *(const float4 *)(wr + k);
            acc = mfma(av.x, bv.x, acc); acc = mfma(av.y, bv.y, acc); acc = mfma(av.z, bv.z, acc); acc = mfma(av.w, bv.w, acc);
        }
        const float bb = a.bi[c0 + l];
#pragma unroll
        for (int r = 0; r < 4; ++r) HL[4 * q + r][c0 + l] = acc[r] + bb;
    }
    __syncthreads();
    // ---- the raw latent leaves: wave wv owns rows 4 wv .. 4 wv + 3
    for (int rr = 4 * wv; rr < 4 * wv + 4; ++rr) {
        const int64_t row = r0 + rr;
        if (row < m) a.lat[row * SLAT + lane] = HL[rr][lane];
    }
    __syncthreads();
    // ---- logits = a2 Wc^T + bc: column tiles wv, wv + 4, ...
    const int nct = (C + 15) / 16;
    for (int t = wv; t < nct; t += 4) {
        const int c0 = 16 * t;
        const int cc = min(c0 + l, C - 1);
        const float *wr = a.Wc + (int64_t)cc * SH2;
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < SH2 / 16; ++c) {
            const int k = 16 * c + 4 * q;
            const float4 av = *(const float4 *)&A2[l][k];
            const float4 bv = *(const float4 *)(wr + k);
            acc = mfma(av.x, bv.x, acc); acc = mfma(av.y, bv.y, acc); acc = mfma(av.z, bv.z, acc); acc = mfma(av.w, bv.w, acc);
        }
        const float bb = a.bc[cc];
#pragma unroll
        for (int r = 0; r < 4; ++r) HL[4 * q + r][c0 + l] = acc[r] + bb;
    }
    __syncthreads();
    // ---- softmax, its largest value and where: a row per wave at a time
    for (int rr = 4 * wv; rr < 4 * wv + 4; ++rr) {
        const int row = r0 + rr;
        if (row < m) mid_dev::softmax_row_top(mid_dev::load_logits(HL[rr], lane, C), row, lane, C, a.z, a.prob, a.unit);
    }
}

}  // namespace

extern "C" {

int idl_small_predict_l1(const float *x, const float *W1, int m, int F, float *a1, void *stream)
{
    IDL_REQUIRE(x && W1 && a1, "small_predict_l1: NULL buffer");
    IDL_REQUIRE(m >= 1 && F >= 4 && (F % 4) == 0, "small_predict_l1: m >= 1, F >= 4 and a multiple of 4");
    IDL_REQUIRE((((uintptr_t)x | (uintptr_t)W1) & 15u) == 0, "small_predict_l1: x / W1 must be 16-byte aligned");
    IDL_REQUIRE(idl::take_plan() == nullptr, "small_predict_l1: not a recordable launch");
    const int rc = idl::raise_dyn_lds<small_predict_l1_kernel>(P1_LDS_BYTES);
    if (rc != IDL_OK) return rc;
    hipLaunchKernelGGL(small_predict_l1_kernel, dim3((unsigned)((m + P1_ROWS - 1) / P1_ROWS)), dim3(P1_THREADS), P1_LDS_BYTES, (hipStream_t)stream, x, W1,
                       m, F, a1);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

int idl_small_predict_mid(const float *a1, const float *b1, const float *W2, const float *b2, const float *Wi, const float *bi, const float *Wc,
                          const float *bc, int m, int C, float *lat, float *z, float *prob, int32_t *unit, void *stream)
{
    IDL_REQUIRE(a1 && b1 && W2 && b2 && Wi && bi && Wc && bc && lat && prob && unit, "small_predict_mid: NULL buffer");
    IDL_REQUIRE(m >= 1 && C >= 1 && C <= SMAX_C, "small_predict_mid: m >= 1, n_clusters in 1..256");
    IDL_REQUIRE((((uintptr_t)a1 | (uintptr_t)b1 | (uintptr_t)W2 | (uintptr_t)Wi | (uintptr_t)Wc) & 15u) == 0,
                "small_predict_mid: a1 / b1 / W2 / Wi / Wc must be 16-byte aligned");
    IDL_REQUIRE(idl::take_plan() == nullptr, "small_predict_mid: not a recordable launch");
    SmallPredictArgs a{a1, b1, W2, b2, Wi, bi, Wc, bc, m, C, lat, z, prob, unit};
    hipLaunchKernelGGL(small_predict_mid_kernel, dim3((unsigned)((m + 15) / 16)), dim3(256), 0, (hipStream_t)stream, a);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

}  // extern "C"
