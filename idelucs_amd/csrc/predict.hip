// predict.hip -- the eval forward of NetLinear behind layer 1, on this library's own launches: what IID_model.predict / calculate_probs and a saved ensemble's
// assign run after idl_l1_fwd when they are asked for predict='native' (idelucs_amd/predict_native.py).
//
// Reference: idelucs/PytorchUtils.py:38-50 in eval mode (both Dropouts are the identity), called at idelucs/models.py:158-170.
//   r1 = ReLU(a1 + b1); lat = r1 W2^T + b2; z = softmax(ReLU(lat) W3^T + b3); prob = max z, unit = argmax z
// The stages are mid_fwd_device.h's with train = 0, in the order and on the tiles of train_step.hip's mid_fwd_body<true>: z and max(lat, 0) have the bits of
// idl_mid_fwd_gather(a1_transposed = 1, train = 0).  What differs: a1_t is only read (r1 lives in registers), the raw latent is stored instead of
// f / inv / r2, and the row's largest z and its class leave with it.
// A row's outputs are a function of that row of a1_t and of the weights alone: row l of an MFMA tile takes its A operand from lane l's registers only, every
// K-slice is added in the same ascending order whatever the tile, and the per-row stages run one row a wave.
#include "common.h"
#include "mid_fwd_device.h"

namespace {

using mid_dev::H1;
using mid_dev::H2;
using mid_dev::MAX_CPL;
using mid_dev::WAVES;
using mid_dev::f32x4_t;

__global__ __launch_bounds__(64 * WAVES) void predict_mid_kernel(const float *__restrict__ a1_t, const float *__restrict__ b1, const float *__restrict__ W2,
                                                                 const float *__restrict__ b2, const float *__restrict__ W3, const float *__restrict__ b3,
                                                                 int m, int C, float *__restrict__ lat, float *__restrict__ z, float *__restrict__ prob,
                                                                 int32_t *__restrict__ unit)
{
    // part[wave][row][col'], col' = (col + 16 (row >> 2)) & 63, then the r2 tile and the logits tile in the same memory: mid_fwd_body's layout
    __shared__ float part[WAVES][16][H2];
    float (*R2t)[H2 + 4] = (float (*)[H2 + 4])&part[0][0][0];               // [16][68]
    float (*LG)[64 * MAX_CPL + 1] = (float (*)[64 * MAX_CPL + 1])&part[2][0][0];   // [16][257]
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l = lane & 15, q = lane >> 4;
    const int r0 = (int)blockIdx.x * 16;                 // m % 16 == 0: every row of the tile is a row of the batch
    const int k0 = 32 * wv + 8 * q;                      // this lane's 8 consecutive k of row r0 + l
    // ---- every global read of the kernel is issued here, before the first dependent instruction
    const float *srcT = a1_t + (int64_t)k0 * m + r0 + l; // element (row r0 + l, column k0 + i) of the transposed image: srcT[i * m]
    float t8[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) t8[i] = srcT[(int64_t)i * m];
    const float4 bb[2] = {*(const float4 *)(b1 + k0), *(const float4 *)(b1 + k0 + 4)};
    mid_dev::W2Tile bw[4];
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) bw[ct] = mid_dev::load_w2(W2, ct, l, k0);
    const int nct = (C + 15) / 16;                       // column tiles of the logits; wave wv < nct owns tile wv
    float4 w3f[4];
    float b3v = 0.f;
    if (wv < nct) mid_dev::load_w3(w3f, b3v, W3, b3, wv, l, q, C);
    const float b2v = b2[lane];
    // ---- r1 = ReLU(a1 + b1), in registers; lat = r1 W2^T: this wave's K-slice
    {
    mid_dev::R1Frag a;
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        float4 v = make_float4(t8[4 * i], t8[4 * i + 1], t8[4 * i + 2], t8[4 * i + 3]);
        v.x += bb[i].x; v.y += bb[i].y; v.z += bb[i].z; v.w += bb[i].w;
        v = mid_dev::relu_dropout4(v, 0, 1u, 0, 0, 0u);
        a.k[4 * i] = v.x; a.k[4 * i + 1] = v.y; a.k[4 * i + 2] = v.z; a.k[4 * i + 3] = v.w;
    }
#pragma unroll
    for (int ct = 0; ct < 4; ++ct) {
        const f32x4_t acc = mid_dev::kslice_tile(a, bw[ct]);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) part[wv][4 * q + reg][(16 * ct + l + 16 * q) & 63] = acc[reg];   // C/D: row = 4q+reg, col = l
    }
    __syncthreads();
    }
    // ---- wave wv owns row wv of the tile: b2 + the 16 K-slices in ascending order is the latent; ReLU
    const int cs = (lane + 16 * (wv >> 2)) & 63;
    const float x = mid_dev::add_slices(b2v, &part[0][wv][cs], 16 * H2);
    const int row = r0 + wv;
    lat[(int64_t)row * H2 + lane] = x;
    const float ar = mid_dev::relu_dropout_latent(x, row, lane, 0, 0, 0u);
    __syncthreads();                             // part is dead
    R2t[wv][lane] = ar;
    __syncthreads();
    // ---- logits tile wv = r2[16 x 64] W3[16 wv .. 16 wv + 15]^T + b3
    if (wv < nct) {
        const f32x4_t acc = mid_dev::logits_tile(R2t, w3f, l, q);
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) LG[4 * q + reg][16 * wv + l] = acc[reg] + b3v;
    }
    __syncthreads();
    // ---- softmax of row wv, its largest value and where
    mid_dev::softmax_row_top(mid_dev::load_logits(LG[wv], lane, C), row, lane, C, z, prob, unit);
}

}  // namespace

extern "C" {

int idl_predict_mid(const float *a1_t, const float *b1, const float *W2, const float *b2, const float *W3, const float *b3, int m, int C,
                    float *lat, float *z, float *prob, int32_t *unit, void *stream)
{
    IDL_REQUIRE(a1_t && b1 && W2 && b2 && W3 && b3 && lat && prob && unit, "predict_mid: NULL buffer");
    IDL_REQUIRE(m >= 16 && (m % 16) == 0 && C >= 1 && C <= 64 * MAX_CPL, "predict_mid: m must be a multiple of 16, n_clusters in 1..256");
    IDL_REQUIRE((((uintptr_t)b1 | (uintptr_t)W2 | (uintptr_t)W3) & 15u) == 0, "predict_mid: b1 / W2 / W3 must be 16-byte aligned");
    IDL_REQUIRE(idl::take_plan() == nullptr, "predict_mid: not a recordable launch");
    hipLaunchKernelGGL(predict_mid_kernel, dim3((unsigned)(m / 16)), dim3(64 * WAVES), 0, (hipStream_t)stream, a1_t, b1, W2, b2, W3, b3, m, C, lat, z,
                       prob, unit);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

}  // extern "C"
