// small_step.hip -- the explicit training step of model_size='small' (myNet, reference idelucs/PytorchUtils.py:6-31) with RMSprop
// (reference models.py:88, :117-133), on this library's own fp32 MFMA tiles (v_mfma_f32_16x16x4_f32).
//
// myNet:  a1 = Dropout(ReLU(x W1^T + b1))            [m, 400]   Linear(F', 400), ReLU, Dropout(0.5)
//         a2 = LeakyReLU(a1 W2^T + b2)               [m, 128]   Linear(400, 128), LeakyReLU(0.01)
//         h  = a2 Wi^T + bi                          [m, 64]    instance head (the latent)
//         z  = Softmax(Dropout(a2) Wc^T + bc)        [m, C]     classifier
//
// One full-batch step is at most 8 launches (python: idelucs_amd/fused_small.py):
//   small_l1_fwd      a1' = x W1^T                              (eight waves a workgroup split K, added up through LDS)
//   small_mid_fwd     bias + ReLU + Dropout of layer 1 in place, a2, d2 = Dropout(a2), f = h / |h|, inv, z      (16 rows a workgroup)
//   InfoNCE / IIC     the existing launches of nce_fused.hip / train_step.hip on f and z (2 launches; 4 for n_clusters > 48)
//   small_mid_bwd     dlogits, dh, da2 = (dd2 + dh Wi) LeakyReLU', dr1 = (da2 W2) ReLU'/Dropout'    (16 rows a workgroup)
//   small_wgrad_rms   every weight gradient as A^T B tiles with the RMSprop update in their epilogue (the gradient stays in registers),
//                     the four bias gradients as column sums with the update behind them, the step loss and step counter, and the
//                     assembly of the NEXT batch into the other x buffer
//                     (small_wgrad_rms_momentum: the same launch with torch's momentum buffer in the update, for RMSprop under
//                     CyclicLR's cycle_momentum; small_wgrad_opt: the same launch with torch's SGD or Adam, models.py:89-92)
//
// Dropout: Philox4x32-10 keyed by the seed, counter (element group, layer, ctl[0]).  Layer ids 11 (after layer 1) and 12 (classifier)
// are distinct from NetLinear's 1 and 2.  The layer-1 mask is recovered in the backward from the sign of a1 (kept and active <=> a1 > 0,
// as NetLinear's kernels do); the classifier's acts on LeakyReLU outputs, which can be negative, so the backward draws it again.
// No atomics anywhere: every sum runs in a fixed order, so a replayed graph reproduces eager launches bit for bit.
#include "common.h"
#include "opt_update_device.h"
#include "philox_device.h"
#include "scaler_device.h"
#include "step_args.h"
#include "wave_ops.h"

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));
using idl_dev::U4;
using idl_dev::philox;

constexpr int SH1 = 400;          // myNet's hidden widths
constexpr int SH2 = 128;
constexpr int SLAT = 64;          // latent (instance head)
constexpr int SMAX_C = 256;
constexpr uint32_t LAYER_A1 = 11u, LAYER_D2 = 12u;
constexpr float SLOPE = 0.01f;    // nn.LeakyReLU() default

__device__ __forceinline__ f32x4_t mfma(float a, float b, f32x4_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

// Dropout(0.5) keep bit of a1[row][col] (layer 1): one Philox draw per group of four consecutive elements of the flat [m, 400] array
__device__ __forceinline__ bool keep_a1(int64_t row, int col, uint32_t step, uint64_t seed)
{
    const int64_t e = row * SH1 + col, g = e >> 2;
    const U4 r = philox((uint32_t)g, LAYER_A1, step, (uint32_t)(g >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t w = (e & 3) == 0 ? r.x : (e & 3) == 1 ? r.y : (e & 3) == 2 ? r.z : r.w;
    return (w >> 31) != 0u;
}

// ... of the classifier's input d2[row][col]: one draw per row, its 128 bits are the row's 128 columns
__device__ __forceinline__ bool keep_d2(int64_t row, int col, uint32_t step, uint64_t seed)
{
    const U4 r = philox((uint32_t)row, LAYER_D2, step, (uint32_t)(row >> 32), (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint32_t w = col < 32 ? r.x : col < 64 ? r.y : col < 96 ? r.z : r.w;
    return ((w >> (col & 31)) & 1u) != 0u;
}

// ---------------------------------------------------------------- layer-1 forward: a1'[m, 400] = x W1^T (bias: small_mid_fwd)
// A workgroup of 8 waves owns 16 rows x 80 units; wave w takes the w-th eighth of K = F in 16-wide chunks in which lane group q
// holds the four consecutive k 4q..4q+3 of its row (one float4 of x and of each W1 row), then the eight partial tiles are added
// in LDS in wave order.  Any F >= 1: a chunk that crosses F (or F % 4 != 0) is read element by element with the tail zeroed.
constexpr int L1_WAVES = 8, L1_CB = 5;
constexpr int L1_THREADS = 64 * L1_WAVES;

__global__ __launch_bounds__(L1_THREADS) void small_l1_fwd_kernel(const float *__restrict__ x, const float *__restrict__ W1, int m, int F,
                                                                  float *__restrict__ a1)
{
    __shared__ float red[L1_WAVES - 1][L1_CB][4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l = lane & 15, q = lane >> 4;
    const int tiles_n = SH1 / (16 * L1_CB);
    const int i0 = ((int)blockIdx.x / tiles_n) * 16, j0 = ((int)blockIdx.x % tiles_n) * 16 * L1_CB;
    const int nch = (F + 15) / 16, c0 = wv * nch / L1_WAVES, c1 = (wv + 1) * nch / L1_WAVES;
    const int row = min(i0 + l, m - 1);                 // (rows past m are computed and not stored)
    const float *xa = x + (int64_t)row * F;
    const float *wb[L1_CB];
#pragma unroll
    for (int cb = 0; cb < L1_CB; ++cb) wb[cb] = W1 + (int64_t)(j0 + 16 * cb + l) * F;
    f32x4_t acc[L1_CB];
#pragma unroll
    for (int cb = 0; cb < L1_CB; ++cb) acc[cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    const bool vec = (F & 3) == 0;
    for (int c = c0; c < c1; ++c) {
        const int k = 16 * c + 4 * q;
        float4 a, b[L1_CB];
        if (vec && k + 4 <= F) {
            a = *(const float4 *)(xa + k);
#pragma unroll
            for (int cb = 0; cb < L1_CB; ++cb) b[cb] = *(const float4 *)(wb[cb] + k);
        } else {
            float t[4], u[L1_CB][4];
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                const bool ok = k + s < F;
                t[s] = ok ? xa[k + s] : 0.f;
#pragma unroll
                for (int cb = 0; cb < L1_CB; ++cb) u[cb][s] = ok ? wb[cb][k + s] : 0.f;
            }
            a = make_float4(t[0], t[1], t[2], t[3]);
#pragma unroll
            for (int cb = 0; cb < L1_CB; ++cb) b[cb] = make_float4(u[cb][0], u[cb][1], u[cb][2], u[cb][3]);
        }
#pragma unroll
        for (int cb = 0; cb < L1_CB; ++cb) {
            acc[cb] = mfma(a.x, b[cb].x, acc[cb]);
            acc[cb] = mfma(a.y, b[cb].y, acc[cb]);
            acc[cb] = mfma(a.z, b[cb].z, acc[cb]);
            acc[cb] = mfma(a.w, b[cb].w, acc[cb]);
        }
    }
    if (wv > 0) {
#pragma unroll
        for (int cb = 0; cb < L1_CB; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) red[wv - 1][cb][r][lane] = acc[cb][r];
    }
    __syncthreads();
    if (wv != 0) return;
#pragma unroll
    for (int cb = 0; cb < L1_CB; ++cb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float s = acc[cb][r];
            for (int w = 0; w < L1_WAVES - 1; ++w) s += red[w][cb][r][lane];
            const int i = i0 + 4 * q + r;                   // C/D: row 4q + r, column l
            if (i < m) a1[(int64_t)i * SH1 + j0 + 16 * cb + l] = s;
        }
}

// ---------------------------------------------------------------- middle forward: 16 rows a workgroup of 4 waves
struct SmallFwdArgs {
    float *a1; const float *b1, *W2, *b2, *Wi, *bi, *Wc, *bc;
    int m, C, train; uint64_t seed; const int64_t *ctl;
    float *a2, *d2, *f, *inv, *z;
};

__global__ __launch_bounds__(256) void small_mid_fwd_kernel(SmallFwdArgs a)
{
    __shared__ float A1[16][SH1 + 4];
    __shared__ float A2[16][SH2 + 4];
    __shared__ float D2[16][SH2 + 4];
    __shared__ float HL[16][SMAX_C + 4];       // the latent, then the logits
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l = lane & 15, q = lane >> 4;
    const int r0 = (int)blockIdx.x * 16, m = a.m, C = a.C;
    const uint32_t step = (uint32_t)a.ctl[0];
    // ---- layer 1: + b1, ReLU, Dropout, in place (rows past m: zeros in LDS)
    for (int e = tid; e < 16 * (SH1 / 4); e += 256) {
        const int rr = e / (SH1 / 4), c = 4 * (e % (SH1 / 4));
        const int64_t row = r0 + rr;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (row < m) {
            float4 *p = (float4 *)(a.a1 + row * SH1 + c);
            v = *p;
            const float4 bb = *(const float4 *)(a.b1 + c);
            v.x += bb.x; v.y += bb.y; v.z += bb.z; v.w += bb.w;
            float s0 = 1.f, s1 = 1.f, s2 = 1.f, s3 = 1.f;
            if (a.train) {
                const int64_t g = (row * SH1 + c) >> 2;
                const U4 r = philox((uint32_t)g, LAYER_A1, step, (uint32_t)(g >> 32), (uint32_t)a.seed, (uint32_t)(a.seed >> 32));
                s0 = (r.x >> 31) ? 2.f : 0.f; s1 = (r.y >> 31) ? 2.f : 0.f; s2 = (r.z >> 31) ? 2.f : 0.f; s3 = (r.w >> 31) ? 2.f : 0.f;
            }
            v.x = v.x > 0.f ? v.x * s0 : 0.f; v.y = v.y > 0.f ? v.y * s1 : 0.f;
            v.z = v.z > 0.f ? v.z * s2 : 0.f; v.w = v.w > 0.f ? v.w * s3 : 0.f;
            *p = v;
        }
        *(float4 *)&A1[rr][c] = v;
    }
    __syncthreads();
    // ---- a2 = LeakyReLU(a1 W2^T + b2): wave wv owns column tiles 2 wv, 2 wv + 1; lane group q holds k = 16 c + 4q .. + 3
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
            const int rr = 4 * q + r;
            const int64_t row = r0 + rr;
            const float v = acc[r] + bb;
            const float y = v > 0.f ? v : SLOPE * v;
            const float d = a.train ? (keep_d2(row, col, step, a.seed) ? 2.f * y : 0.f) : y;
            A2[rr][col] = y;
            D2[rr][col] = d;
            if (row < m) { a.a2[row * SH2 + col] = y; a.d2[row * SH2 + col] = d; }
        }
    }
    __syncthreads();
    // ---- h = a2 Wi^T + bi: wave wv owns latent columns 16 wv .. 16 wv + 15
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
    // ---- f = h / max(|h|, 1e-12), inv (LossFunctions.py:79): wave wv owns rows 4 wv .. 4 wv + 3
    for (int rr = 4 * wv; rr < 4 * wv + 4; ++rr) {
        const float x = HL[rr][lane];
        const float nrm = fmaxf(sqrtf(idl_dev::wave_sum_f(x * x)), 1e-12f);
        const int64_t row = r0 + rr;
        if (row < m) {
            a.f[row * SLAT + lane] = x / nrm;
            if (lane == 0) a.inv[row] = 1.f / nrm;
        }
    }
    __syncthreads();
    // ---- logits = d2 Wc^T + bc: column tiles wv, wv + 4, ...
    const int nct = (C + 15) / 16;
    for (int t = wv; t < nct; t += 4) {
        const int c0 = 16 * t;
        const int cc = min(c0 + l, C - 1);
        const float *wr = a.Wc + (int64_t)cc * SH2;
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < SH2 / 16; ++c) {
            const int k = 16 * c + 4 * q;
            const float4 av = *(const float4 *)&D2[l][k];
            const float4 bv = *(const float4 *)(wr + k);
            acc = mfma(av.x, bv.x, acc); acc = mfma(av.y, bv.y, acc); acc = mfma(av.z, bv.z, acc); acc = mfma(av.w, bv.w, acc);
        }
        const float bb = a.bc[cc];
#pragma unroll
        for (int r = 0; r < 4; ++r) HL[4 * q + r][c0 + l] = acc[r] + bb;
    }
    __syncthreads();
    // ---- softmax, a row per wave at a time
    for (int rr = 4 * wv; rr < 4 * wv + 4; ++rr) {
        const int64_t row = r0 + rr;
        float lg[4];
        float mx = -INFINITY;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = 64 * t + lane;
            lg[t] = c < C ? HL[rr][c] : -INFINITY;
            mx = fmaxf(mx, lg[t]);
        }
        mx = idl_dev::wave_max_f(mx);
        float den = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = 64 * t + lane;
            if (c < C) { lg[t] = __expf(lg[t] - mx); den += lg[t]; }
        }
        den = idl_dev::wave_sum_f(den);
        if (row < m) {
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int c = 64 * t + lane;
                if (c < C) a.z[row * C + c] = lg[t] / den;
            }
        }
    }
}

// ---------------------------------------------------------------- middle backward: 16 rows a workgroup of 4 waves
struct SmallBwdArgs {
    const float *z, *f, *inv, *G; int g_parts; const float *dP0, *dzs;
    const float *a1, *a2, *W2, *Wi, *Wc;
    int m, C, train; float nce_coef; uint64_t seed; int64_t *ctl; int64_t batch_advance;
    float *dlogits, *dh, *da2, *dr1;
};

__global__ __launch_bounds__(256) void small_mid_bwd_kernel(SmallBwdArgs a)
{
    __shared__ float DL[16][SMAX_C + 4];
    __shared__ float DH[16][SLAT + 4];
    __shared__ float DA[16][SH2 + 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, l = lane & 15, q = lane >> 4;
    const int r0 = (int)blockIdx.x * 16, m = a.m, C = a.C, B = a.m / 2;
    const uint32_t step = (uint32_t)a.ctl[0];
    // dP0 (n_clusters <= 48) and the partner rows of z in LDS: the per-row product z_partner dP0 then reads no global memory
    __shared__ float DP[48 * 48];
    __shared__ float ZP[16][48];
    const bool lds_dp = a.dzs == nullptr && C <= 48;
    if (lds_dp) {
        for (int e = tid; e < C * C; e += 256) DP[e] = a.dP0[e];
        for (int e = tid; e < 16 * C; e += 256) {
            const int rr = e / C, row = r0 + rr;
            ZP[rr][e % C] = row < m ? a.z[(int64_t)(row < B ? row + B : row - B) * C + e % C] : 0.f;
        }
        __syncthreads();
    }
    // ---- per row: softmax backward of the IIC gradient (dlogits) and the normalise backward of the InfoNCE gradient (dh)
    for (int rr = 4 * wv; rr < 4 * wv + 4; ++rr) {
        const int row = r0 + rr;
        if (row >= m) {                              // (wave-uniform)
            for (int c = lane; c < SMAX_C; c += 64) DL[rr][c] = 0.f;
            DH[rr][lane] = 0.f;
            continue;
        }
        const int prow = row < B ? row + B : row - B;
        float zc[4], dz[4];
        float dot = 0.f;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = 64 * t + lane;
            zc[t] = 0.f; dz[t] = 0.f;
            if (c < C) {
                zc[t] = a.z[(int64_t)row * C + c];
                float acc = 0.f;
                if (a.dzs != nullptr) acc = a.dzs[(int64_t)prow * C + c];      // z dP0 of the partner row (dP0 is symmetric)
                else if (lds_dp) for (int k = 0; k < C; ++k) acc = fmaf(ZP[rr][k], DP[k * C + c], acc);
                else for (int k = 0; k < C; ++k) acc = fmaf(a.z[(int64_t)prow * C + k], a.dP0[(int64_t)k * C + c], acc);
                dz[t] = acc;
                dot += acc * zc[t];
            }
        }
        dot = idl_dev::wave_sum_f(dot);
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int c = 64 * t + lane;
            const float dl = c < C ? zc[t] * (dz[t] - dot) : 0.f;
            if (c < C) a.dlogits[(int64_t)row * C + c] = dl;
            DL[rr][c] = dl;
        }
        const float fr = a.f[(int64_t)row * SLAT + lane];
        float gs = a.G[(int64_t)row * SLAT + lane];
        for (int p = 1; p < a.g_parts; ++p) gs += a.G[((int64_t)p * m + row) * SLAT + lane];
        const float df = a.nce_coef * (gs - 2.f * a.f[(int64_t)prow * SLAT + lane]);
        const float proj = idl_dev::wave_sum_f(fr * df);
        const float dh = (df - fr * proj) * a.inv[row];
        a.dh[(int64_t)row * SLAT + lane] = dh;
        DH[rr][lane] = dh;
    }
    __syncthreads();
    // ---- da2 = (Dropout'(dlogits Wc) + dh Wi) LeakyReLU': wave wv owns column tiles 2 wv, 2 wv + 1
    for (int t = 0; t < 2; ++t) {
        const int c0 = 16 * (2 * wv + t), col = c0 + l;
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f}, aci = {0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < C; k += 4) {             // B[k][j] = Wc[k][j]
            const int kk = k + q;
            const float av = kk < C ? DL[l][kk] : 0.f;
            const float bv = kk < C ? a.Wc[(int64_t)kk * SH2 + col] : 0.f;
            acc = mfma(av, bv, acc);
        }
        float bi[SLAT / 4];
#pragma unroll
        for (int k = 0; k < SLAT; k += 4) bi[k / 4] = a.Wi[(int64_t)(k + q) * SH2 + col];
#pragma unroll
        for (int k = 0; k < SLAT; k += 4) aci = mfma(DH[l][k + q], bi[k / 4], aci);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int rr = 4 * q + r;
            const int64_t row = r0 + rr;
            float v = 0.f;
            if (row < m) {
                const float dd2 = a.train ? (keep_d2(row, col, step, a.seed) ? 2.f * acc[r] : 0.f) : acc[r];
                const float y = a.a2[row * SH2 + col];
                v = (dd2 + aci[r]) * (y > 0.f ? 1.f : SLOPE);
                a.da2[row * SH2 + col] = v;
            }
            DA[rr][col] = v;
        }
    }
    __syncthreads();
    // ---- dr1 = (da2 W2) * ReLU'/Dropout' (kept and active <=> a1 > 0): column tiles wv, wv + 4, ... of 25
    const float s1 = a.train ? 2.f : 1.f;
    for (int t = wv; t < SH1 / 16; t += 4) {
        const int col = 16 * t + l;
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        float bw[SH2 / 4];                           // every B operand of the tile requested before the first product
#pragma unroll
        for (int k = 0; k < SH2; k += 4) bw[k / 4] = a.W2[(int64_t)(k + q) * SH1 + col];
#pragma unroll
        for (int k = 0; k < SH2; k += 4) acc = mfma(DA[l][k + q], bw[k / 4], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t row = r0 + 4 * q + r;
            if (row < m) a.dr1[row * SH1 + col] = a.a1[row * SH1 + col] > 0.f ? s1 * acc[r] : 0.f;
        }
    }
    if (blockIdx.x == 0 && tid == 0 && a.batch_advance != 0) a.ctl[1] += a.batch_advance;
}

// ---------------------------------------------------------------- weight gradients + RMSprop + step loss + next batch, one launch
// Workgroups of 8 waves.  Roles, in block order:
//   gradient tiles of W1, W2, Wi, Wc: out[M, N] = dy^T xin (dy [m, M], xin [m, N] row-major, the contraction index m as the ROW, which
//     is the MFMA operand map) as 32 x 64 tiles; the 8 waves split K = m, add up through LDS in wave order, and wave 0 applies RMSprop
//     to the tile from its registers (g = grad + wd W; v = alpha v + (1 - alpha) g^2; W -= lr g / (sqrt(v) + eps): torch.optim.RMSprop)
//   bias columns of b1, b2, bi, bc: 64 columns a workgroup, column sums of dy over m in a fixed order, then RMSprop
//   one workgroup: the step loss (out[2] = mean(loss_rows), out[0] = w_nce out[2] + w_iic out[3], out[1] += out[0]) and ctl[0] += 1
//   the next batch (idl_gather_pairs_at at ctl[1], which small_mid_bwd advanced), two 256-thread gather tiles a workgroup
constexpr int WG_WAVES = 8, WG_RB = 2, WG_CB = 4;
constexpr int WG_THREADS = 64 * WG_WAVES;
constexpr int WG_TM = 16 * WG_RB, WG_TN = 16 * WG_CB;
constexpr int BIAS_COLS = 64;

struct GradJob { const float *dy, *xin; int M, N, tiles_n; float *W, *v, *grad; };
struct BiasJob { const float *dy; int N; float *b, *v, *grad; };
struct SmallWgArgs {
    GradJob g[4]; int g_end[4];
    BiasJob b[4]; int b_end[4];
    int loss_blk, gather_end;
    int m; const float *hyper; int64_t *ctl;
    const float *loss_rows; float w_nce, w_iic; float *out;
    idl_dev::GatherArgs gth;
};

__device__ __forceinline__ void rms(float g, float &p, float &v, const float *h)
{
    const float gi = g + h[3] * p;                    // grad.add(param, alpha=weight_decay)
    v = v * h[1] + h[4] * gi * gi;                    // square_avg.mul_(alpha).addcmul_(g, g, value=1-alpha)
    p = p - h[0] * (gi / (sqrtf(v) + h[2]));          // param.addcdiv_(grad, sqrt(v)+eps, value=-lr)
}

// RMSprop with the momentum buffer that CyclicLR's cycle_momentum gives the optimizer (models.py:87-88 under models.py:99): torch's order,
// buf = mu buf + g / (sqrt(v) + eps); p -= lr buf, mu = h[5] (mu = 0: buf = g / avg, the momentum-free step)
__device__ __forceinline__ void rms_momentum(float g, float &p, float &v, float &buf, const float *h)
{
    const float gi = g + h[3] * p;
    v = v * h[1] + h[4] * gi * gi;
    buf = buf * h[5] + gi / (sqrtf(v) + h[2]);        // buf.mul_(momentum).addcdiv_(grad, avg)
    p = p - h[0] * buf;                               // param.add_(buf, alpha=-lr)
}

// The four kernels of this launch (RMSprop, RMSprop with momentum, SGD, Adam) differ in the update of one element and in nothing else.
// What they share is written once, below: grad_tile_sum (operand loads, product loop, cross-wave reduction, C/D index map),
// bias_cols_sum (the bias column sums) and loss_or_gather (step loss, step counter, next batch).  The per-element update is a callable
// epi(e, g), called once per owned element e with its summed gradient g, behind the optional grad[e] = g store.
// What stays in each __global__ function: its __shared__ array, its by-value struct parameters and the role dispatch (the two unrolled
// loops over a.g[t] / a.b[t]).  A shared body that takes SmallWgArgs by reference and holds the dispatch was tried: the argument block
// is then copied to scratch (the RMSprop kernels: 124 VGPRs and 616 / 680 bytes of scratch a lane, against 118 and 0 as written here).
// The epilogue callables capture POINTERS BY VALUE (W, v, buf, st1, st2, hyper, copied into locals inside the role's branch first; the
// Coef may be captured by reference): one that reads j.W through a captured GradJob & makes the compiler load the kernel argument again
// for every element (31 more scalar loads and 32 more waits a kernel).  loss_or_gather's after() runs once in one thread and may read
// the kernel's struct parameter directly.
template <class Epi>
__device__ __forceinline__ void grad_tile_sum(const GradJob &j, int t, int m, float *lds, Epi epi)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l = lane & 15, q = lane >> 4;
    const int i0 = (t / j.tiles_n) * WG_TM, j0 = (t % j.tiles_n) * WG_TN;
    const int ks = (m + 3) / 4, s0 = wv * ks / WG_WAVES, s1 = (wv + 1) * ks / WG_WAVES;
    int ia[WG_RB], jb[WG_CB];
#pragma unroll
    for (int rb = 0; rb < WG_RB; ++rb) ia[rb] = min(i0 + 16 * rb + l, j.M - 1);
#pragma unroll
    for (int cb = 0; cb < WG_CB; ++cb) jb[cb] = min(j0 + 16 * cb + l, j.N - 1);
    f32x4_t acc[WG_RB][WG_CB];
#pragma unroll
    for (int rb = 0; rb < WG_RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < WG_CB; ++cb) acc[rb][cb] = f32x4_t{0.f, 0.f, 0.f, 0.f};
    // eight K-steps' operands are requested before their products (clamped rows, not predicated loads: a step past this wave's
    // share reads a valid row and contributes zero through A)
    constexpr int U = 8;
    for (int s = s0; s < s1; s += U) {
        float av[U][WG_RB], bv[U][WG_CB];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = 4 * (s + u) + q;
            const bool ok = s + u < s1 && k < m;
            const int kr = min(k, m - 1);
#pragma unroll
            for (int rb = 0; rb < WG_RB; ++rb) {
                const float t = j.dy[(int64_t)kr * j.M + ia[rb]];
                av[u][rb] = ok ? t : 0.f;
            }
#pragma unroll
            for (int cb = 0; cb < WG_CB; ++cb) bv[u][cb] = j.xin[(int64_t)kr * j.N + jb[cb]];
        }
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int rb = 0; rb < WG_RB; ++rb)
#pragma unroll
                for (int cb = 0; cb < WG_CB; ++cb) acc[rb][cb] = mfma(av[u][rb], bv[u][cb], acc[rb][cb]);
    }
    float (*red)[WG_RB * WG_CB][4][64] = (float (*)[WG_RB * WG_CB][4][64])lds;
    if (wv > 0) {
#pragma unroll
        for (int rb = 0; rb < WG_RB; ++rb)
#pragma unroll
            for (int cb = 0; cb < WG_CB; ++cb)
#pragma unroll
                for (int r = 0; r < 4; ++r) red[wv - 1][rb * WG_CB + cb][r][lane] = acc[rb][cb][r];
    }
    __syncthreads();
    if (wv != 0) return;
#pragma unroll
    for (int rb = 0; rb < WG_RB; ++rb)
#pragma unroll
        for (int cb = 0; cb < WG_CB; ++cb)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float g = acc[rb][cb][r];
                for (int w = 0; w < WG_WAVES - 1; ++w) g += red[w][rb * WG_CB + cb][r][lane];
                const int i = i0 + 16 * rb + 4 * q + r, jj = j0 + 16 * cb + l;       // C/D: row 4q + r, column l
                if (i < j.M && jj < j.N) {
                    const int64_t e = (int64_t)i * j.N + jj;
                    if (j.grad != nullptr) j.grad[e] = g;
                    epi(e, g);
                }
            }
}

template <class Epi>
__device__ __forceinline__ void bias_cols_sum(const BiasJob &j, int t, int m, float *lds, Epi epi)
{
    const int tid = threadIdx.x, c = tid & (BIAS_COLS - 1), rg = tid / BIAS_COLS;       // 8 row groups
    const int col = t * BIAS_COLS + c;
    const int ccol = min(col, j.N - 1);
    float s = 0.f;
    for (int r = rg; r < m; r += WG_THREADS / BIAS_COLS) s += j.dy[(int64_t)r * j.N + ccol];
    float (*red)[BIAS_COLS] = (float (*)[BIAS_COLS])lds;
    red[rg][c] = s;
    __syncthreads();
    if (rg != 0 || col >= j.N) return;
    float g = red[0][c];
    for (int w = 1; w < WG_THREADS / BIAS_COLS; ++w) g += red[w][c];
    if (j.grad != nullptr) j.grad[col] = g;
    epi(col, g);
}

// The update of element e of one tensor: parameter and state loads, the update, the stores in the order W then v (RMSprop), states then
// parameter (SGD / Adam).  (MOM: the momentum form, buf = the tensor's momentum_buffer.)
template <bool MOM, class I>
__device__ __forceinline__ void rms_at(float *P, float *V, float *buf, I e, float g, const float *hyper)
{
    float p = P[e], v = V[e];
    if constexpr (MOM) {
        float bu = buf[e];
        rms_momentum(g, p, v, bu, hyper);
        buf[e] = bu;
    } else {
        rms(g, p, v, hyper);
    }
    P[e] = p; V[e] = v;
}

// opt_update<KIND> of opt_update_device.h (KIND 1: SGD with momentum and weight decay, 2: Adam) on (g, p, state1, state2)
template <int KIND, class I>
__device__ __forceinline__ void opt_at(float *P, float *st1, float *st2, I e, float g, const idl_dev::Coef<KIND> &c)
{
    float p = P[e], a = st1[e], b = 0.f;
    if constexpr (KIND == idl_dev::KIND_ADAM) b = st2[e];
    idl_dev::opt_update<KIND>(g, p, a, b, c);
    st1[e] = a;
    if constexpr (KIND == idl_dev::KIND_ADAM) st2[e] = b;
    P[e] = p;
}

// The blocks behind the bias columns: the step loss and ctl[0] += 1 in one wave of one workgroup, then the gather rider.  after() runs
// in the ONE thread that advances ctl[0].
template <class After>
__device__ __forceinline__ void loss_or_gather(const SmallWgArgs &a, int bid, After after)
{
    if (bid == a.loss_blk) {
        if (threadIdx.x >= 64) return;
        const int lane = threadIdx.x;
        float s = 0.f;
        if (a.loss_rows != nullptr)
            for (int r = lane; r < a.m; r += 64) s += a.loss_rows[r];
        s = idl_dev::wave_sum_f(s);
        if (lane == 0) {
            if (a.loss_rows != nullptr) {
                const float nce = s / (float)a.m;
                const float tot = a.w_nce * nce + a.w_iic * a.out[3];
                a.out[2] = nce; a.out[0] = tot; a.out[1] += tot;
            }
            a.ctl[0] += 1;
            after();
        }
        return;
    }
    const int blk = 2 * (bid - a.loss_blk - 1) + (int)(threadIdx.x >> 8);
    if (blk < a.gather_end) idl_dev::gather_block(a.gth, (int64_t)blk, (int)(threadIdx.x & 255));
}

struct MomBufs { float *g[4], *b[4]; };               // momentum_buffer of the four weights / the four biases

__global__ __launch_bounds__(WG_THREADS) void small_wgrad_rms_kernel(SmallWgArgs a)
{
    __shared__ float lds[(WG_WAVES - 1) * WG_RB * WG_CB * 256];
    const int bid = (int)blockIdx.x;
    int lo = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (bid < a.g_end[t]) {
            float *const W = a.g[t].W, *const v = a.g[t].v;
            const float *const hyper = a.hyper;
            grad_tile_sum(a.g[t], bid - lo, a.m, lds, [=](int64_t e, float g) { rms_at<false>(W, v, (float *)nullptr, e, g, hyper); });
            return;
        }
        lo = a.g_end[t];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (bid < a.b_end[t]) {
            float *const b = a.b[t].b, *const v = a.b[t].v;
            const float *const hyper = a.hyper;
            bias_cols_sum(a.b[t], bid - lo, a.m, lds, [=](int col, float g) { rms_at<false>(b, v, (float *)nullptr, col, g, hyper); });
            return;
        }
        lo = a.b_end[t];
    }
    loss_or_gather(a, bid, [] {});
}

// The momentum form of the launch above: the same grid and roles, one more stream (momentum_buffer) per tensor.
__global__ __launch_bounds__(WG_THREADS) void small_wgrad_momentum_kernel(SmallWgArgs a, MomBufs mb)
{
    __shared__ float lds[(WG_WAVES - 1) * WG_RB * WG_CB * 256];
    const int bid = (int)blockIdx.x;
    int lo = 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (bid < a.g_end[t]) {
            float *const W = a.g[t].W, *const v = a.g[t].v, *const buf = mb.g[t];
            const float *const hyper = a.hyper;
            grad_tile_sum(a.g[t], bid - lo, a.m, lds, [=](int64_t e, float g) { rms_at<true>(W, v, buf, e, g, hyper); });
            return;
        }
        lo = a.g_end[t];
    }
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        if (bid < a.b_end[t]) {
            float *const b = a.b[t].b, *const v = a.b[t].v, *const buf = mb.b[t];
            const float *const hyper = a.hyper;
            bias_cols_sum(a.b[t], bid - lo, a.m, lds, [=](int col, float g) { rms_at<true>(b, v, buf, col, g, hyper); });
            return;
        }
        lo = a.b_end[t];
    }
    loss_or_gather(a, bid, [] {});
}

// ---------------------------------------------------------------- the last launch with torch's SGD or Adam (models.py:89-92)
// small_wgrad_opt_kernel<KIND>: the grid, roles and block order of small_wgrad_rms_kernel; the epilogue is opt_at<KIND>, its coefficients
// from a DEVICE double[5] (make_coef: Adam's bias corrections in double).  Adam's step count is the optimizer's own, not ctl[0] (the
// dropout counter, which restarts with every voter): every workgroup that updates reads *step_in, and the ONE thread that advances ctl[0]
// writes *step_in + 1 to *step_out, a different word -- no word read in this launch is written in it (not all workgroups are resident
// before the first one ends).
struct OptBufs {
    float *g1[4], *b1[4];             // SGD: momentum_buffer, Adam: exp_avg, of the four weights / the four biases
    float *g2[4], *b2[4];             // Adam: exp_avg_sq
    const double *hyper;
    const int64_t *step_in;
    int64_t *step_out;
};

// (a.hyper, RMSprop's float hyperparameters, is not read here; GradJob::v / BiasJob::v, RMSprop's running averages, are not either: the
//  states come in ob.)
template <int KIND>
__global__ __launch_bounds__(WG_THREADS) void small_wgrad_opt_kernel(SmallWgArgs a, OptBufs ob)
{
    __shared__ float lds[(WG_WAVES - 1) * WG_RB * WG_CB * 256];
    const int bid = (int)blockIdx.x;
    if (bid < a.b_end[3]) {
        const idl_dev::Coef<KIND> c = idl_dev::make_coef<KIND>(ob.hyper, ob.step_in);
        int lo = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (bid < a.g_end[t]) {
                float *const W = a.g[t].W, *const st1 = ob.g1[t], *const st2 = ob.g2[t];
                grad_tile_sum(a.g[t], bid - lo, a.m, lds, [=, &c](int64_t e, float g) { opt_at<KIND>(W, st1, st2, e, g, c); });
                return;
            }
            lo = a.g_end[t];
        }
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            if (bid < a.b_end[t]) {
                float *const b = a.b[t].b, *const st1 = ob.b1[t], *const st2 = ob.b2[t];
                bias_cols_sum(a.b[t], bid - lo, a.m, lds, [=, &c](int col, float g) { opt_at<KIND>(b, st1, st2, col, g, c); });
                return;
            }
            lo = a.b_end[t];
        }
    }
    loss_or_gather(a, bid, [&ob] { *ob.step_out = *ob.step_in + 1; });
}

// ---------------------------------------------------------------- the two dropout masks of a step (tests)
__global__ __launch_bounds__(256) void small_masks_kernel(uint64_t seed, uint32_t step, int m, float *mask1, float *mask2)
{
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t n1 = (int64_t)m * SH1, n2 = (int64_t)m * SH2;
    if (e < n1) mask1[e] = keep_a1(e / SH1, (int)(e % SH1), step, seed) ? 1.f : 0.f;
    if (e < n2) mask2[e] = keep_d2(e / SH2, (int)(e % SH2), step, seed) ? 1.f : 0.f;
}

}  // namespace

extern "C" {

int idl_small_l1_fwd(const float *x, const float *W1, int m, int F, float *a1, void *stream)
{
    IDL_REQUIRE(x && W1 && a1, "NULL buffer");
    IDL_REQUIRE(m >= 1 && F >= 1, "small_l1_fwd: m and F must be >= 1");
    const int tiles = ((m + 15) / 16) * (SH1 / (16 * L1_CB));
    hipLaunchKernelGGL(small_l1_fwd_kernel, dim3((unsigned)tiles), dim3(L1_THREADS), 0, (hipStream_t)stream, x, W1, m, F, a1);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

int idl_small_mid_fwd(float *a1, const float *b1, const float *W2, const float *b2, const float *Wi, const float *bi, const float *Wc,
                      const float *bc, int m, int C, int train, uint64_t seed, const int64_t *ctl, float *a2, float *d2, float *f,
                      float *inv, float *z, void *stream)
{
    IDL_REQUIRE(a1 && b1 && W2 && b2 && Wi && bi && Wc && bc && ctl && a2 && d2 && f && inv && z, "NULL buffer");
    IDL_REQUIRE(m >= 1 && C >= 1 && C <= SMAX_C, "small_mid_fwd: m >= 1, n_clusters in 1..256");
    SmallFwdArgs a{a1, b1, W2, b2, Wi, bi, Wc, bc, m, C, train ? 1 : 0, seed, ctl, a2, d2, f, inv, z};
    hipLaunchKernelGGL(small_mid_fwd_kernel, dim3((unsigned)((m + 15) / 16)), dim3(256), 0, (hipStream_t)stream, a);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

int idl_small_mid_bwd(const float *z, const float *f, const float *inv, const float *G, int g_parts, const float *dP0, const float *dzs,
                      const float *a1, const float *a2, const float *W2, const float *Wi, const float *Wc, int m, int C, int train,
                      float nce_coef, uint64_t seed, int64_t *ctl, int64_t batch_advance, float *dlogits, float *dh, float *da2,
                      float *dr1, void *stream)
{
    IDL_REQUIRE(z && f && inv && G && (dP0 || dzs) && a1 && a2 && W2 && Wi && Wc && ctl && dlogits && dh && da2 && dr1, "NULL buffer");
    IDL_REQUIRE(m >= 2 && (m % 2) == 0 && C >= 1 && C <= SMAX_C && g_parts >= 1 && g_parts <= 16,
                "small_mid_bwd: even m, n_clusters in 1..256, g_parts in 1..16");
    SmallBwdArgs a{z, f, inv, G, g_parts, dP0, dzs, a1, a2, W2, Wi, Wc, m, C, train ? 1 : 0, nce_coef, seed, ctl, batch_advance,
                   dlogits, dh, da2, dr1};
    hipLaunchKernelGGL(small_mid_bwd_kernel, dim3((unsigned)((m + 15) / 16)), dim3(256), 0, (hipStream_t)stream, a);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

// What every form of the step's last launch takes from `x` on.
struct SmallStepIn {
    const float *x, *dr1, *a1, *da2, *a2, *dh, *d2, *dlogits; int m, F, C; const float *loss_rows; float w_nce, w_iic; float *out;
    const idl_next_batch_t *next_batch; void *stream;
};

// The forms of the step's last launch share everything but the optimizer's epilogue: momentum_buffer == NULL is idl_small_wgrad_rms;
// opt != NULL (checked by the caller) is idl_small_wgrad_opt (SGD / Adam: its states, hyperparameters and step words; square_avg and hyper are not looked at).
static int small_wgrad_launch(float *const *params, float *const *grads, float *const *square_avg, float *const *momentum_buffer,
                              const float *hyper, int64_t *ctl, const SmallStepIn &s, const idl_opt_state_t *opt = nullptr)
{
    const int m = s.m, F = s.F, C = s.C;
    IDL_REQUIRE(params && (opt != nullptr || (square_avg && hyper)) && ctl && s.x && s.dr1 && s.a1 && s.da2 && s.a2 && s.dh && s.d2 && s.dlogits, "NULL buffer");
    IDL_REQUIRE(m >= 1 && F >= 1 && C >= 1 && C <= SMAX_C, "small_wgrad_rms: m, F >= 1, n_clusters in 1..256");
    for (int t = 0; t < 8; ++t) IDL_REQUIRE(params[t] && (opt != nullptr || square_avg[t]), "small_wgrad_rms: NULL parameter or running average");
    SmallWgArgs a{};
    if (const int rc = idl_step::whole_batch_of("small_wgrad_rms", s.next_batch, ctl, a.gth)) return rc;
    IDL_REQUIRE(a.gth.y == nullptr || a.gth.f == F, "small_wgrad_rms: the next batch's rows must have width F (next_batch->f)");
    const float *dys[4] = {s.dr1, s.da2, s.dh, s.dlogits}, *xs[4] = {s.x, s.a1, s.a2, s.d2};
    const int Ms[4] = {SH1, SH2, SLAT, C}, Ns[4] = {F, SH1, SH2, SH2};
    int end = 0;
    for (int t = 0; t < 4; ++t) {
        GradJob &j = a.g[t];
        j.dy = dys[t]; j.xin = xs[t]; j.M = Ms[t]; j.N = Ns[t]; j.tiles_n = (Ns[t] + WG_TN - 1) / WG_TN;
        j.W = params[2 * t]; j.v = opt == nullptr ? square_avg[2 * t] : nullptr; j.grad = grads ? grads[2 * t] : nullptr;
        end += ((Ms[t] + WG_TM - 1) / WG_TM) * j.tiles_n;
        a.g_end[t] = end;
    }
    for (int t = 0; t < 4; ++t) {
        BiasJob &j = a.b[t];
        j.dy = dys[t]; j.N = Ms[t]; j.b = params[2 * t + 1]; j.v = opt == nullptr ? square_avg[2 * t + 1] : nullptr; j.grad = grads ? grads[2 * t + 1] : nullptr;
        end += (Ms[t] + BIAS_COLS - 1) / BIAS_COLS;
        a.b_end[t] = end;
    }
    a.loss_blk = end++;
    a.m = m; a.hyper = hyper; a.ctl = ctl; a.loss_rows = s.loss_rows; a.w_nce = s.w_nce; a.w_iic = s.w_iic; a.out = s.out;
    IDL_REQUIRE(s.loss_rows == nullptr || s.out != nullptr, "small_wgrad_rms: the step loss needs out");
    a.gather_end = 0;
    if (a.gth.y != nullptr) {
        a.gather_end = (int)idl_dev::gather_blocks(a.gth.f, a.gth.batch);
        end += (a.gather_end + 1) / 2;
    }
    const dim3 grid((unsigned)end), block(WG_THREADS);
    const hipStream_t stream = (hipStream_t)s.stream;
    if (opt != nullptr) {
        OptBufs ob{};
        for (int t = 0; t < 4; ++t) {
            ob.g1[t] = opt->state1[2 * t]; ob.b1[t] = opt->state1[2 * t + 1];
            if (opt->kind == idl_dev::KIND_ADAM) { ob.g2[t] = opt->state2[2 * t]; ob.b2[t] = opt->state2[2 * t + 1]; }
        }
        ob.hyper = opt->hyper; ob.step_in = opt->step_in; ob.step_out = opt->step_out;
        if (opt->kind == idl_dev::KIND_SGD) hipLaunchKernelGGL(small_wgrad_opt_kernel<idl_dev::KIND_SGD>, grid, block, 0, stream, a, ob);
        else hipLaunchKernelGGL(small_wgrad_opt_kernel<idl_dev::KIND_ADAM>, grid, block, 0, stream, a, ob);
    } else if (momentum_buffer != nullptr) {
        MomBufs mb{};
        for (int t = 0; t < 4; ++t) {
            IDL_REQUIRE(momentum_buffer[2 * t] && momentum_buffer[2 * t + 1], "small_wgrad_rms_momentum: NULL momentum buffer");
            mb.g[t] = momentum_buffer[2 * t]; mb.b[t] = momentum_buffer[2 * t + 1];
        }
        hipLaunchKernelGGL(small_wgrad_momentum_kernel, grid, block, 0, stream, a, mb);
    } else {
        hipLaunchKernelGGL(small_wgrad_rms_kernel, grid, block, 0, stream, a);
    }
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

int idl_small_wgrad_rms(float *const *params, float *const *grads, float *const *square_avg, const float *hyper, int64_t *ctl,
                        const float *x, const float *dr1, const float *a1, const float *da2, const float *a2, const float *dh,
                        const float *d2, const float *dlogits, int m, int F, int C, const float *loss_rows, float w_nce, float w_iic,
                        float *out, const idl_next_batch_t *next_batch, void *stream)
{
    return small_wgrad_launch(params, grads, square_avg, nullptr, hyper, ctl,
                              SmallStepIn{x, dr1, a1, da2, a2, dh, d2, dlogits, m, F, C, loss_rows, w_nce, w_iic, out, next_batch, stream});
}

int idl_small_wgrad_rms_momentum(float *const *params, float *const *grads, float *const *square_avg, float *const *momentum_buffer,
                                 const float *hyper, int64_t *ctl,
                                 const float *x, const float *dr1, const float *a1, const float *da2, const float *a2, const float *dh,
                                 const float *d2, const float *dlogits, int m, int F, int C, const float *loss_rows, float w_nce, float w_iic,
                                 float *out, const idl_next_batch_t *next_batch, void *stream)
{
    IDL_REQUIRE(momentum_buffer != nullptr, "small_wgrad_rms_momentum: NULL momentum buffers");
    return small_wgrad_launch(params, grads, square_avg, momentum_buffer, hyper, ctl,
                              SmallStepIn{x, dr1, a1, da2, a2, dh, d2, dlogits, m, F, C, loss_rows, w_nce, w_iic, out, next_batch, stream});
}

int idl_small_wgrad_opt(const idl_opt_state_t *opt, float *const *params, float *const *grads, int64_t *ctl,
                        const float *x, const float *dr1, const float *a1, const float *da2, const float *a2, const float *dh,
                        const float *d2, const float *dlogits, int m, int F, int C, const float *loss_rows, float w_nce, float w_iic,
                        float *out, const idl_next_batch_t *next_batch, void *stream)
{
    if (const int rc = idl_step::opt_state_of("small_wgrad_opt", opt, ctl, 1u << idl_dev::KIND_SGD | 1u << idl_dev::KIND_ADAM, 8)) return rc;
    return small_wgrad_launch(params, grads, nullptr, nullptr, nullptr, ctl,
                              SmallStepIn{x, dr1, a1, da2, a2, dh, d2, dlogits, m, F, C, loss_rows, w_nce, w_iic, out, next_batch, stream}, opt);
}


int idl_small_dropout_masks(uint64_t seed, int64_t step, int m, float *mask1, float *mask2, void *stream)
{
    IDL_REQUIRE(mask1 && mask2 && m >= 1, "small_dropout_masks: NULL buffer or m < 1");
    const int64_t n = (int64_t)m * SH1;
    hipLaunchKernelGGL(small_masks_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, (uint32_t)step, m, mask1, mask2);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

}  // extern "C"
