// The tile of out[M x N] = A^T B (nce_fused.hip: at_b_kernel, at_b_batched_kernel), as text: both kernels are this body on their own arguments -- A, lda, B, ldb,
// K, M, N, out, ldo in scope, tile (blockIdx.x, blockIdx.y) -- so that the lone voter's kernel stays the code it was when the batched one joined it (as a
// __device__ function inlined into both, the compiler schedules the loads of the lone kernel differently: 7.6 us against 5.8 at 200 classes).
    __shared__ float part[3][64][4];
    const int tid = threadIdx.x, wv = tid >> 6, lane = tid & 63, l = lane & 15, q = lane >> 4;
    const int c1 = blockIdx.x * 16, c2 = blockIdx.y * 16;
    const bool ok1 = c1 + l < M, ok2 = c2 + l < N;
    f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
    for (int kb = 128 * wv; kb < K; kb += 512) {             // the contraction index is dealt to the four waves in blocks of 128 (32 MFMA steps, every load in flight first)
        const float *pa = A + (ok1 ? c1 + l : 0), *pb = B + (ok2 ? c2 + l : 0);
        float av[32], bv[32];
#pragma unroll
        for (int u = 0; u < 32; ++u) {                       // (clamped, not predicated)
            const int k = kb + 4 * u + q, kk = k < K ? k : K - 1;
            av[u] = pa[(size_t)kk * lda]; bv[u] = pb[(size_t)kk * ldb];
        }
#pragma unroll
        for (int u = 0; u < 32; u += 2) {
            const bool in0 = kb + 4 * u + q < K, in1 = kb + 4 * (u + 1) + q < K;
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32((ok1 && in0) ? av[u] : 0.f, (ok2 && in0) ? bv[u] : 0.f, acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32((ok1 && in1) ? av[u + 1] : 0.f, (ok2 && in1) ? bv[u + 1] : 0.f, acc1, 0, 0, 0);
        }
    }
    f32x4 acc = acc0 + acc1;
    if (wv > 0) { part[wv - 1][lane][0] = acc[0]; part[wv - 1][lane][1] = acc[1]; part[wv - 1][lane][2] = acc[2]; part[wv - 1][lane][3] = acc[3]; }
    __syncthreads();
    if (wv == 0 && ok2) {
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int r = c1 + 4 * q + reg;
            if (r < M) out[(size_t)r * ldo + c2 + l] = ((acc[reg] + part[0][lane][reg]) + part[1][lane][reg]) + part[2][lane][reg];
        }
    }
