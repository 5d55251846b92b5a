// opt_step.hip -- the last launch of a NetLinear training step whose optimizer is SGD with momentum, Adam (reference
// idelucs/models.py:89-92, stepped at models.py:131-132) or RMSprop with the momentum buffer that CyclicLR's cycle_momentum gives it
// (models.py:87-88 under models.py:99): idl_opt_step_gather_wgrad, the counterpart of idl_rmsprop_step
// (train_step.hip) with the optimizer generalised.  The forward, the backward and the loss launches in front of it do not know
// which optimizer follows them; this file is where the two enter the step.
//
// Grid, as the RMSprop launch's: [dW2 tiles][next-batch gather blocks][streaming optimizer blocks], 256 threads each.
//   dW2 tiles       one 16 x 16 tile of wg_dy^T wg_x each on the fp32 matrix cores (v_mfma_f32_16x16x4_f32), the four waves splitting
//                   the contraction index, partial tiles added through LDS in a fixed order, the update applied from registers
//   gather blocks   idl_dev::gather_block: the optional rider that assembles the next batch
//   optimizer       every other tensor: 16-byte accesses, four elements' loads of every stream in flight before the first use;
//                   tensors whose gradient arrives as stacked partials (bias gradients, dW3 at n_clusters <= 48) per element, the
//                   partials summed in ascending order
// Nothing is accumulated with atomics: every sum runs in a fixed order, a replayed step equals the eager one bit for bit.
//
// Hyperparameters are a DEVICE double[5] = {lr, momentum | beta1, beta2 | alpha, eps, weight_decay}: a captured graph follows what a
// scheduler changed between epochs, and Adam's bias corrections 1 - beta^t are formed in double as torch forms them on the host
// (an fp32 1 - 0.999^t is 3e-5 off at t = 1, which a bias tensor that starts at zero shows in full).
// Adam's step count is the optimizer's own (not ctl[0], the dropout counter, which restarts with every voter): every workgroup
// reads *step_in and ONE thread writes *step_in + 1 to *step_out, a different word -- no word that a workgroup of this launch reads
// is written in this launch (not all workgroups are resident before the first one ends).  The caller swaps the two words from step
// to step.
#include <string.h>

#include "common.h"
#include "opt_update_device.h"
#include "scaler_device.h"
#include "step_args.h"
#include "wave_ops.h"

namespace {

typedef float f32x4_t __attribute__((ext_vector_type(4)));

constexpr int OPT_THREADS = 256;
constexpr int OPT_UNROLL = 4;          // 16-byte elements per thread of the streaming update
constexpr int OPT_MAX_BLOCKS = 1024;   // optimizer blocks of one tensor (beyond: a block walks on)
constexpr int PART_CHUNK = 16;         // stacked partial gradients requested together
// (Coef, make_coef and opt_update -- the arithmetic of the three optimizers -- are opt_update_device.h's: small_step.hip's last launch shares them)
using idl_dev::Coef; using idl_dev::make_coef; using idl_dev::opt_update;
using idl_dev::KIND_SGD; using idl_dev::KIND_ADAM; using idl_dev::KIND_RMSPROP;

struct OptArgs {
    const float *loss_rows;   // optional step-loss assembly (models.py:128), as idl_rmsprop_step
    float *out;
    int loss_m;
    float w_nce, w_iic;
    float *p[8];
    const float *g[8];
    float *s1[8];             // SGD: momentum_buffer; Adam: exp_avg; RMSprop: square_avg
    float *s2[8];             // Adam: exp_avg_sq; RMSprop: momentum_buffer
    int64_t n[8];
    int parts[8];             // g[t] holds parts[t] stacked partial gradients [parts, n]
    int count;
    const float *wg_dy, *wg_x; float *wg_grad;
    int wg_t, wg_m, wg_n_out, wg_n_in, wg_tiles, wg_xt;      // wg_xt: wg_x is stored transposed, [n_in, wg_m]
    int first[9];             // optimizer blocks [first[t], first[t + 1]) belong to tensor t
    const double *hyper;
    const int64_t *step_in;
    int64_t *step_out;
    int64_t *ctl;
    int64_t batch_advance;
};

// One 16 x 16 tile of dy^T x: the four waves take a quarter of the contraction index each.  red: 1024 floats of LDS.
// (The operand loops are dyT_x_tile16.inc, shared with train_step.hip's wgrad_tile_rms.  The LDS reduction here, and the streaming body and
//  step-loss tail of opt_step_kernel below, follow wgrad_tile_rms and rmsprop_body as separate texts: merging them would move that file's
//  kernels, which their register, ISA and bit-for-bit tests pin.)
template <int KIND>
__device__ __forceinline__ void wgrad_tile(const OptArgs &a, int tile, const Coef<KIND> &c, float *red, const int tid)
{
    const int lane = tid & 63, wv = tid >> 6, l = lane & 15, q = lane >> 4;
    const int tn = a.wg_n_in / 16;
    const int i0 = (tile / tn) * 16, j0 = (tile % tn) * 16;
    const int lda = a.wg_n_out, ldb = a.wg_n_in, m = a.wg_m;
    const int per = ((m + 15) / 16) * 4;                     // rows per wave, a multiple of 4
    const int kb = wv * per, ke = (kb + per < m) ? kb + per : m;
    f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
    const float *pa = a.wg_dy + i0 + l, *pb = a.wg_x + j0 + l;    // A[i = l][k = q] = dy[k][i0 + l], B[k = q][j = l] = x[k][j0 + l]
    constexpr bool AHEAD = false;                            // (no look-ahead form here: the streaming blocks want the registers)
#include "dyT_x_tile16.inc"
    const int o = (i0 + (tid >> 4)) * ldb + j0 + (tid & 15);      // this thread's element of the tile in the epilogue
    float *p = a.p[a.wg_t], *s1 = a.s1[a.wg_t], *s2 = a.s2[a.wg_t];
    float pi = p[o], ai = s1[o], bi = KIND != KIND_SGD ? s2[o] : 0.f;      // (requested before the barrier: beside the LDS round trip)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wv * 256 + (4 * q + r) * 16 + l] = acc[r];          // C/D: row = 4 q + reg, col = l
    __syncthreads();
    const float g = (red[tid] + red[256 + tid]) + (red[512 + tid] + red[768 + tid]);
    if (a.wg_grad != nullptr) a.wg_grad[o] = g;
    opt_update<KIND>(g, pi, ai, bi, c);
    s1[o] = ai;
    if constexpr (KIND != KIND_SGD) s2[o] = bi;
    p[o] = pi;
}

template <int KIND>
__global__ __launch_bounds__(OPT_THREADS) void opt_step_kernel(OptArgs a, int n_gather, idl_dev::GatherArgs g)
{
    const int blk = (int)blockIdx.x, tix = (int)threadIdx.x;
    // grid order: the weight-gradient tiles (dependent chains of strided loads: first, so that the streaming blocks behind them hide
    // their latency), then the gather blocks, then the optimizer blocks
    const int b0 = blk - a.wg_tiles;
    if (b0 >= 0 && b0 < n_gather) {
        idl_dev::gather_block(g, (int64_t)b0, tix);
        return;
    }
    const Coef<KIND> c = make_coef<KIND>(a.hyper, a.step_in);
    if (blk < a.wg_tiles) {
        __shared__ float red[1024];
        wgrad_tile<KIND>(a, blk, c, red, tix);
        return;
    }
    const int bid = b0 - n_gather;
    int t = 0;
    while (t + 1 < a.count && bid >= a.first[t + 1]) ++t;
    const int bx = bid - a.first[t], gx = a.first[t + 1] - a.first[t];
    if (gx > 0) {
        float *p = a.p[t]; const float *gr = a.g[t]; float *s1 = a.s1[t]; float *s2 = a.s2[t];
        const int64_t n = a.n[t];
        const uintptr_t al = ((uintptr_t)p) | ((uintptr_t)gr) | ((uintptr_t)s1) | (KIND != KIND_SGD ? (uintptr_t)s2 : 0);
        if (a.parts[t] == 1 && (n & 3) == 0 && (al & 15u) == 0) {
            float4 *p4 = (float4 *)p; const float4 *g4 = (const float4 *)gr; float4 *a4 = (float4 *)s1; float4 *b4 = (float4 *)s2;
            const int64_t n4 = n / 4, stride = (int64_t)gx * OPT_THREADS;
            for (int64_t i = (int64_t)bx * OPT_THREADS + tix; i < n4; i += OPT_UNROLL * stride) {
                float4 pv[OPT_UNROLL], gv[OPT_UNROLL], av[OPT_UNROLL], bv[OPT_UNROLL];
#pragma unroll
                for (int u = 0; u < OPT_UNROLL; ++u) {
                    const int64_t iu = i + u * stride < n4 ? i + u * stride : i;        // clamped, not predicated: the loads stay unconditional
                    pv[u] = p4[iu]; gv[u] = g4[iu]; av[u] = a4[iu];
                    if constexpr (KIND != KIND_SGD) bv[u] = b4[iu]; else bv[u] = float4{0.f, 0.f, 0.f, 0.f};
                }
#pragma unroll
                for (int u = 0; u < OPT_UNROLL; ++u) {
                    if (i + u * stride < n4) {
                        opt_update<KIND>(gv[u].x, pv[u].x, av[u].x, bv[u].x, c); opt_update<KIND>(gv[u].y, pv[u].y, av[u].y, bv[u].y, c);
                        opt_update<KIND>(gv[u].z, pv[u].z, av[u].z, bv[u].z, c); opt_update<KIND>(gv[u].w, pv[u].w, av[u].w, bv[u].w, c);
                        a4[i + u * stride] = av[u];
                        if constexpr (KIND != KIND_SGD) b4[i + u * stride] = bv[u];
                        p4[i + u * stride] = pv[u];
                    }
                }
            }
        } else {
            const int parts = a.parts[t];
            for (int64_t i = (int64_t)bx * OPT_THREADS + tix; i < n; i += (int64_t)gx * OPT_THREADS) {
                float pi = p[i], ai = s1[i], bi = KIND != KIND_SGD ? s2[i] : 0.f;
                float sum = gr[i];
                for (int q0 = 1; q0 < parts; q0 += PART_CHUNK) {      // PART_CHUNK independent loads in flight, added in ascending order
                    float part[PART_CHUNK];
#pragma unroll
                    for (int q = 0; q < PART_CHUNK; ++q) part[q] = gr[(int64_t)(q0 + q < parts ? q0 + q : q0) * n + i];
#pragma unroll
                    for (int q = 0; q < PART_CHUNK; ++q) if (q0 + q < parts) sum += part[q];
                }
                opt_update<KIND>(sum, pi, ai, bi, c);
                s1[i] = ai;
                if constexpr (KIND != KIND_SGD) s2[i] = bi;
                p[i] = pi;
            }
        }
    }
    if (bid == 0 && tix == 0) {
        // (ctl[1] is what the gather blocks of this launch read: it moves here only in a launch without them -- the launcher sees to it)
        a.ctl[0] += 1;
        if (a.batch_advance != 0) a.ctl[1] += a.batch_advance;
        *a.step_out = *a.step_in + 1;
    }
    if (a.out != nullptr && bid == a.first[a.count] - 1 && tix < 64) {
        // step loss = w_nce * mean(loss_rows) + w_iic * IIC (left in out[3] by the IIC core); out[1] = running sum
        const float iic = a.out[3], run = a.out[1];
        float acc = 0.f;
        for (int i0 = 0; i0 < a.loss_m; i0 += 64 * 16) {      // 16 loads in flight, added in ascending order
            float part[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) { const int i = i0 + tix + 64 * j; part[j] = i < a.loss_m ? a.loss_rows[i] : 0.f; }
#pragma unroll
            for (int j = 0; j < 16; ++j) acc += part[j];
        }
        acc = idl_dev::wave_sum_f(acc) / (float)a.loss_m;
        if (tix == 0) { const float l = a.w_nce * acc + a.w_iic * iic; a.out[0] = l; a.out[1] = run + l; a.out[2] = acc; }
    }
}

}  // namespace

extern "C" {

int idl_opt_step_gather_wgrad(const idl_opt_tail_t *tail, const idl_opt_state_t *opt, const idl_next_batch_t *next_batch, void *stream)
{
    IDL_REQUIRE(tail != nullptr, "opt_step: NULL tail");
    const idl_opt_tail_t &t = *tail;
    const int count = t.count, wg_index = t.wg_index;
    IDL_REQUIRE(count >= 1 && count <= 8 && t.params && t.grads && t.sizes && t.ctl, "opt_step: 1..8 tensors");
    IDL_REQUIRE(t.square_avg == nullptr && t.hyper == nullptr, "opt_step: tail->square_avg and tail->hyper must be NULL (the optimizer is opt)");
    IDL_REQUIRE(t.skip_index == -1, "opt_step: tail->skip_index must be -1");
    if (const int rc = idl_step::opt_state_of("opt_step", opt, t.ctl, 1u << KIND_SGD | 1u << KIND_ADAM | 1u << KIND_RMSPROP, count)) return rc;
    const int kind = opt->kind;
    OptArgs a{};
    a.count = count;
    IDL_REQUIRE(t.loss_rows == nullptr || (t.out != nullptr && t.loss_m > 0), "opt_step: tail->loss_rows given without out or with loss_m < 1");
    a.loss_rows = t.loss_rows; a.out = t.loss_rows != nullptr ? t.out : nullptr; a.loss_m = t.loss_m; a.w_nce = t.w_nce; a.w_iic = t.w_iic;
    a.hyper = opt->hyper; a.step_in = opt->step_in; a.step_out = opt->step_out; a.ctl = t.ctl; a.batch_advance = t.batch_advance;
    for (int i = 0; i < count; ++i) {
        a.p[i] = t.params[i]; a.g[i] = t.grads[i]; a.s1[i] = opt->state1[i]; a.s2[i] = kind != KIND_SGD ? opt->state2[i] : nullptr; a.n[i] = t.sizes[i];
        a.parts[i] = t.grad_parts ? t.grad_parts[i] : 1;
        IDL_REQUIRE(a.parts[i] >= 1 && t.sizes[i] >= 0, "opt_step: tail->grad_parts must be >= 1, sizes >= 0");
        IDL_REQUIRE(t.sizes[i] == 0 || a.p[i], "opt_step: a tensor without its parameter pointer");
        IDL_REQUIRE(t.sizes[i] == 0 || i == wg_index || a.g[i], "opt_step: a tensor without its gradient");
    }
    if (wg_index >= 0) {
        IDL_REQUIRE(wg_index < count && t.wg_dy && t.wg_x && t.wg_m >= 1 && t.wg_n_out >= 16 && (t.wg_n_out % 16) == 0 && t.wg_n_in >= 16 &&
                    (t.wg_n_in % 16) == 0 && t.sizes[wg_index] == (int64_t)t.wg_n_out * t.wg_n_in && (int64_t)t.wg_m * t.wg_n_in < (1ll << 31) &&
                    (int64_t)t.wg_m * t.wg_n_out < (1ll << 31),
                    "opt_step: in-launch weight gradient needs n_out, n_in multiples of 16 and sizes[wg_index] == n_out * n_in");
        IDL_REQUIRE(!t.wg_x_transposed || ((t.wg_m & 3) == 0 && (((uintptr_t)t.wg_x) & 15u) == 0), "opt_step: transposed wg_x needs 4 | m and 16-byte alignment");
        a.wg_t = wg_index; a.wg_dy = t.wg_dy; a.wg_x = t.wg_x; a.wg_grad = t.wg_grad; a.wg_m = t.wg_m; a.wg_n_out = t.wg_n_out; a.wg_n_in = t.wg_n_in;
        a.wg_tiles = (t.wg_n_out / 16) * (t.wg_n_in / 16);
        a.wg_xt = t.wg_x_transposed ? 1 : 0;
        a.n[wg_index] = 0;                  // its optimizer blocks have nothing to do: the tile workgroups update it
    }
    idl_dev::GatherArgs g{};
    if (const int rc = idl_step::whole_batch_of("opt_step", next_batch, t.ctl, g)) return rc;
    IDL_REQUIRE(g.y == nullptr || t.batch_advance == 0, "opt_step: the launch that assembles the next batch reads ctl[1] and cannot advance it: tail->batch_advance must be 0");
    int nb_total = 0;
    for (int i = 0; i < count; ++i) {
        const uintptr_t al = ((uintptr_t)a.p[i]) | ((uintptr_t)a.g[i]) | ((uintptr_t)a.s1[i]) | ((uintptr_t)a.s2[i]);
        const bool vec = a.parts[i] == 1 && (a.n[i] & 3) == 0 && (al & 15u) == 0;
        int64_t nb = vec ? (a.n[i] / 4 + OPT_THREADS * OPT_UNROLL - 1) / (OPT_THREADS * OPT_UNROLL) : (a.n[i] + OPT_THREADS - 1) / OPT_THREADS;
        if (nb > OPT_MAX_BLOCKS) nb = OPT_MAX_BLOCKS;
        a.first[i] = nb_total;
        nb_total += (int)nb;
    }
    if (nb_total == 0) nb_total = 1;        // (step counter / loss assembly still need a block)
    for (int i = count; i <= 8; ++i) a.first[i] = nb_total;
    const int64_t extra = g.y != nullptr ? idl_dev::gather_blocks(g.f, g.batch) : 0;
    IDL_REQUIRE(extra + nb_total + a.wg_tiles < (1ll << 30), "opt_step: grid too large");
    const dim3 grid((unsigned)(a.wg_tiles + extra + nb_total)), block(OPT_THREADS);
    if (kind == KIND_SGD) hipLaunchKernelGGL(opt_step_kernel<KIND_SGD>, grid, block, 0, (hipStream_t)stream, a, (int)extra, g);
    else if (kind == KIND_ADAM) hipLaunchKernelGGL(opt_step_kernel<KIND_ADAM>, grid, block, 0, (hipStream_t)stream, a, (int)extra, g);
    else hipLaunchKernelGGL(opt_step_kernel<KIND_RMSPROP>, grid, block, 0, (hipStream_t)stream, a, (int)extra, g);
    IDL_HIP_TRY(hipGetLastError());
    return IDL_OK;
}

}  // extern "C"
