// mid_fwd_device.h -- the stages of the NetLinear step's forward middle (bias, ReLU + Dropout of layer 1, lat = r1 W2^T + b2 on fp32 MFMA over 16 K-slices,
// normalise, ReLU + Dropout of the latent, logits on MFMA, row softmax), each defined once for the kernels of train_step.hip that run them: mid_fwd_body (a
// 16-row tile from a1 in place), sums_fwd_kernel (8 rows straight from layer 1's partial sums) and the unfused pair relu_dropout_fwd_kernel / head_row -- and
// for predict.hip's predict_mid_kernel, the eval forward (train = 0) that leaves the raw latent and the row's largest z instead of f / inv / r2.  The
// tests hold those kernels to each other bit for bit; here is what makes that hold.  What differs between them -- where a lane's eight values come from, where
// r1 goes, which rows of the tile are valid, the LDS layouts -- is written out in each body.
// Operands travel by value, or by references that inlining dissolves, and the loads only load: a body can issue every global read before its first dependent
// instruction.  The cut of each stage is the one that leaves the kernels' instruction streams as they were (DESIGN, History: the table); sums_fwd_kernel sits at
// 128 registers, where another cut of the same arithmetic spills -- compare the resource remarks before and after any change here.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "philox_device.h"
#include "wave_ops.h"

namespace mid_dev {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
constexpr int H1 = 512;       // width of layer 1
constexpr int H2 = 64;        // latent width of NetLinear == one wavefront
constexpr int MAX_CPL = 4;    // classes per lane: n_clusters <= 256
constexpr int WAVES = 16;     // waves of a workgroup == K-slices of lat = r1 W2^T (32 k each)

// ---------------------------------------------------------------- ReLU + Dropout(0.5) of four values at float4 index idx4 of the flat activation
// Philox counter (idx4, layer, step, idx4 >> 32): the sign bit of each word decides one value -- kept and doubled, or dropped.  The mask is never stored (a
// kept, active unit is one whose output is > 0).  A bias is the caller's to add in front.
__device__ __forceinline__ float4 dropout_scale4(int64_t idx4, uint32_t layer, int train, uint64_t seed, uint32_t step)
{
    float s0 = 1.f, s1 = 1.f, s2 = 1.f, s3 = 1.f;
    if (train) {
        const idl_dev::U4 r = idl_dev::philox((uint32_t)idx4, layer, step, (uint32_t)(idx4 >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
        s0 = (r.x >> 31) ? 2.f : 0.f; s1 = (r.y >> 31) ? 2.f : 0.f;
        s2 = (r.z >> 31) ? 2.f : 0.f; s3 = (r.w >> 31) ? 2.f : 0.f;
    }
    return make_float4(s0, s1, s2, s3);
}
__device__ __forceinline__ float4 relu_dropout4(float4 v, int64_t idx4, uint32_t layer, int train, uint64_t seed, uint32_t step)
{
    const float4 s = dropout_scale4(idx4, layer, train, seed, step);
    v.x = v.x > 0.f ? v.x * s.x : 0.f; v.y = v.y > 0.f ? v.y * s.y : 0.f;
    v.z = v.z > 0.f ? v.z * s.z : 0.f; v.w = v.w > 0.f ? v.w * s.w : 0.f;
    return v;
}

// ---------------------------------------------------------------- ReLU + Dropout(0.5) of the latent value x of (row, lane)
// Philox counter (row, 2, step, 0): bit lane of word x serves lanes 0-31, of word y lanes 32-63.
__device__ __forceinline__ float relu_dropout_latent(float x, int row, int lane, int train, uint64_t seed, uint32_t step)
{
    float s = 1.f;
    if (train) {
        const idl_dev::U4 r = idl_dev::philox((uint32_t)row, 2u, step, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
        const uint32_t word = (lane < 32) ? r.x : r.y;
        s = ((word >> (lane & 31)) & 1u) ? 2.f : 0.f;
    }
    return x > 0.f ? x * s : 0.f;
}

// ---------------------------------------------------------------- the fragments (loads only)
// lane = 16 q + l.  W2 of column tile ct of the latent (lat[:, 16 ct .. 16 ct + 15]): B[k][c = l] = W2[16 ct + l][k0 .. k0 + 7], k0 = the lane's first k
struct W2Tile { float4 lo, hi; };
__device__ __forceinline__ W2Tile load_w2(const float *W2, int ct, int l, int k0)
{
    const float4 *wsrc = (const float4 *)(W2 + (int64_t)(16 * ct + l) * H1 + k0);
    return W2Tile{wsrc[0], wsrc[1]};
}
// W3 / b3 of logits tile `tile` (classes 16 tile .. 16 tile + 15, clamped to C - 1): B[k = 16 q + s][c = l] = W3[16 tile + l][16 q + s]
__device__ __forceinline__ void load_w3(float4 (&w)[4], float &b, const float *W3, const float *b3, int tile, int l, int q, int C)
{
    const int c = min(16 * tile + l, C - 1);
    const float4 *wsrc = (const float4 *)(W3 + (int64_t)c * H2 + 16 * q);
#pragma unroll
    for (int i = 0; i < 4; ++i) w[i] = wsrc[i];
    b = b3[c];
}

// ---------------------------------------------------------------- one 16 x 16 tile of a K-slice of lat = r1 W2^T: 8 MFMAs (32 a wave over the four tiles)
// a: the lane's eight consecutive k of r1's row l.  C/D: row = 4 q + reg, column = l.
struct R1Frag { float k[8]; };
__device__ __forceinline__ f32x4_t kslice_tile(R1Frag a, W2Tile b)
{
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.k[0], b.lo.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.k[1], b.lo.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.k[2], b.lo.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.k[3], b.lo.w, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.k[4], b.hi.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.k[5], b.hi.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.k[6], b.hi.z, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a.k[7], b.hi.w, acc, 0, 0, 0);
    return acc;
}

// ---------------------------------------------------------------- one latent row, a wave: this lane's value = b2 + the 16 K-slices in ascending order
// slice0 + w * stride: where the caller's LDS layout keeps slice w's value of (row, lane)
__device__ __forceinline__ float add_slices(float b2v, const float *slice0, int stride)
{
    float x = b2v;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) x += slice0[w * stride];
    return x;
}
// ... and what becomes of it: leaves f = x / max(||x||, 1e-12) (F.normalize(dim=1)), inv and r2 = Dropout(ReLU(x)) of a `valid` row; returns this lane's r2
__device__ __forceinline__ float latent_row(float x, int row, int lane, bool valid, int train, uint64_t seed, uint32_t step,
                                            float *f, float *inv, float *r2)
{
    const float nrm = fmaxf(sqrtf(idl_dev::wave_sum_f(x * x)), 1e-12f);
    const float ar = relu_dropout_latent(x, row, lane, train, seed, step);
    if (valid) {
        f[(int64_t)row * H2 + lane] = x / nrm;
        if (lane == 0) inv[row] = 1.f / nrm;
        r2[(int64_t)row * H2 + lane] = ar;
    }
    return ar;
}

// ---------------------------------------------------------------- logits tile = r2[16 x 64] W3[16 tile .. 16 tile + 15]^T (b3 is the caller's to add): 16 MFMAs
// R2t: the r2 tile in LDS, [16][68].  C/D: row = 4 q + reg, column = l.
__device__ __forceinline__ f32x4_t logits_tile(const float (*R2t)[H2 + 4], const float4 (&w)[4], int l, int q)
{
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 t = *(const float4 *)&R2t[l][16 * q + 4 * i];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(t.x, w[i].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(t.y, w[i].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(t.z, w[i].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(t.w, w[i].w, acc, 0, 0, 0);
    }
    return acc;
}

// ---------------------------------------------------------------- softmax of one row, a wave: lane holds the logits of classes 64 t + lane, t < MAX_CPL
struct RowLogits { float v[MAX_CPL]; };       // -inf beyond C
__device__ __forceinline__ RowLogits load_logits(const float *lgrow, int lane, int C)      // from a row of logits in LDS
{
    RowLogits lg;
#pragma unroll
    for (int t = 0; t < MAX_CPL; ++t) {
        const int c = t * 64 + lane;
        lg.v[t] = c < C ? lgrow[c] : -INFINITY;
    }
    return lg;
}
struct RowSoftmax { RowLogits e; float den; };      // e.v[t] = exp(logit - the row's largest) of class 64 t + lane < C; den = their sum over the row
__device__ __forceinline__ RowSoftmax softmax_terms(RowLogits lg, int lane, int C)
{
    float mx = -INFINITY;
#pragma unroll
    for (int t = 0; t < MAX_CPL; ++t) mx = fmaxf(mx, lg.v[t]);
    mx = idl_dev::wave_max_f(mx);
    float den = 0.f;
#pragma unroll
    for (int t = 0; t < MAX_CPL; ++t) {
        const int c = t * 64 + lane;
        if (c < C) { lg.v[t] = __expf(lg.v[t] - mx); den += lg.v[t]; }
    }
    return RowSoftmax{lg, idl_dev::wave_sum_f(den)};
}
__device__ __forceinline__ void softmax_row(RowLogits lg, int row, int lane, int C, bool valid, float *z)      // z[row][.] is written if `valid`
{
    const RowSoftmax s = softmax_terms(lg, lane, C);
    if (valid) {
#pragma unroll
        for (int t = 0; t < MAX_CPL; ++t) {
            const int c = t * 64 + lane;
            if (c < C) z[(int64_t)row * C + c] = s.e.v[t] / s.den;
        }
    }
}
// ... of the eval forward (predict.hip): the same z (written where z != NULL), prob[row] = the row's largest z and unit[row] = the lowest class that attains
// it (torch.max's choice among equal values; a row whose logits are not numbers leaves prob = -1, unit = C - 1)
__device__ __forceinline__ void softmax_row_top(RowLogits lg, int row, int lane, int C, float *z, float *prob, int32_t *unit)
{
    const RowSoftmax s = softmax_terms(lg, lane, C);
    float zt[MAX_CPL], best = -1.f;
#pragma unroll
    for (int t = 0; t < MAX_CPL; ++t) {
        zt[t] = -1.f;
        if (t * 64 + lane < C) { zt[t] = s.e.v[t] / s.den; best = fmaxf(best, zt[t]); }
    }
    best = idl_dev::wave_max_f(best);
    uint64_t first = (uint64_t)(C - 1);
#pragma unroll
    for (int t = MAX_CPL - 1; t >= 0; --t) {
        const int c = t * 64 + lane;
        if (c < C && zt[t] == best) first = (uint64_t)c;
    }
    first = idl_dev::wave_min_u64(first);
    if (z != nullptr) {
#pragma unroll
        for (int t = 0; t < MAX_CPL; ++t) {
            const int c = t * 64 + lane;
            if (c < C) z[(int64_t)row * C + c] = zt[t];
        }
    }
    if (lane == 0) { prob[row] = best; unit[row] = (int32_t)first; }
}

}  // namespace mid_dev
