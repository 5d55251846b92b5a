// dyT_x_tile16.inc -- the operand loops of one 16 x 16 tile of dy^T x on the fp32 matrix cores (v_mfma_f32_16x16x4_f32): one wave's share
// [kb, ke) of the contraction index, accumulated into acc.  Included as TEXT by train_step.hip's wgrad_tile_rms and opt_step.hip's wgrad_tile,
// in the middle of the function body (an `if ... else if ... else for` chain, nothing else): a function, or an include that also declared
// acc / pa / pb, moves registers and statements in the kernels that inline the tile, whose register, ISA and bit-for-bit tests pin them.
// The includer has in scope:
//   a            the launch's arguments: a.wg_dy [m, lda], a.wg_x ([m, ldb], or [ldb, m] when a.wg_xt), a.wg_xt
//   AHEAD        a COMPILE-TIME constant (a template parameter or a constexpr bool): true adds the form that requests both 128-row batches
//                of a wave's 256 rows before the first product; false drops that branch
//   m, lda, ldb  rows, and the row lengths of dy and x
//   j0, l, q     the tile's first column of x; this lane's column (lane & 15) and k-slot (lane >> 4)
//   kb, ke, per  the wave's rows [kb, ke), ke <= m, and the rows a wave takes (a multiple of 4)
//   pa, pb       a.wg_dy + i0 + l, a.wg_x + j0 + l:  A[i = l][k = q] = dy[k][i0 + l],  B[k = q][j = l] = x[k][j0 + l]
//   acc          f32x4_t, the wave's partial tile (C/D layout: row = 4 q + reg, col = l)
// What stays in the two files, because it differs on purpose: the declarations around the include, the look-ahead loads (train_step.hip),
// the state loads in front of the barrier (opt_step.hip), the LDS reduction and the epilogue.
    if (AHEAD && a.wg_xt && per == 256 && kb + per <= m) {
        const float *pbt = a.wg_x + (int64_t)(j0 + l) * m;
        float av[64], bv[64];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int u4 = 0; u4 < 8; ++u4) {
                const float4 t4 = *(const float4 *)(pbt + kb + 128 * h + 32 * q + 4 * u4);
                bv[32 * h + 4 * u4] = t4.x; bv[32 * h + 4 * u4 + 1] = t4.y; bv[32 * h + 4 * u4 + 2] = t4.z; bv[32 * h + 4 * u4 + 3] = t4.w;
            }
#pragma unroll
            for (int u = 0; u < 32; ++u) av[32 * h + u] = pa[(kb + 128 * h + 32 * q + u) * lda];
        }
#pragma unroll
        for (int u = 0; u < 64; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
    } else if (a.wg_xt && (per & 127) == 0 && kb + per <= m) {
        // x stored transposed ([n_in, m]): lane (l, q) walks 32 consecutive k of ITS column per batch (16-byte reads), and MFMA step
        // u takes k = k0 + 32 q + u on both operands -- any assignment of k to (step, q) is a valid order of the same sum
        const float *pbt = a.wg_x + (int64_t)(j0 + l) * m;
        for (int k0 = kb; k0 < ke; k0 += 128) {
            float av[32], bv[32];
#pragma unroll
            for (int u4 = 0; u4 < 8; ++u4) {
                const float4 t4 = *(const float4 *)(pbt + k0 + 32 * q + 4 * u4);
                bv[4 * u4] = t4.x; bv[4 * u4 + 1] = t4.y; bv[4 * u4 + 2] = t4.z; bv[4 * u4 + 3] = t4.w;
            }
#pragma unroll
            for (int u = 0; u < 32; ++u) av[u] = pa[(k0 + 32 * q + u) * lda];
#pragma unroll
            for (int u = 0; u < 32; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
        }
    } else if (a.wg_xt) {
        for (int k0 = kb; k0 < ke; k0 += 4) {
            const int k = k0 + q;
            const bool ok = k < ke;
            const float ta = ok ? pa[k * lda] : 0.f, tb = ok ? a.wg_x[(int64_t)(j0 + l) * m + k] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(ta, tb, acc, 0, 0, 0);
        }
    } else
    for (int k0 = kb; k0 < ke; k0 += 128) {                  // 64 independent loads in flight per lane, then 32 MFMAs
        float av[32], bv[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) {
            const int k = k0 + 4 * u + q;
            const bool ok = k < ke;
            const int kc = ok ? k : ke - 1;                  // clamped, not predicated: inside the operands, the loads stay unconditional
            const float ta = pa[kc * lda], tb = pb[kc * ldb];
            av[u] = ok ? ta : 0.f;
            bv[u] = ok ? tb : 0.f;
        }
#pragma unroll
        for (int u = 0; u < 32; ++u) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[u], bv[u], acc, 0, 0, 0);
    }
