// store_policy.h -- the cache policy of the training step's bulk output stores.  A plain store leaves its line dirty in the XCD's L2, and the dirty
// lines are written back when the launch ends, in front of the next launch; a write-through store (the sc1 bit) sends the bytes on while the kernel
// still runs, and drops the line from that L2.  Only 16-byte stores are ever write-through: narrower ones are one fabric write each (2.7x / 6x the
// time per byte at 8 / 4 bytes).  No value changes with the policy, and no byte stored through here is read again in the launch that stores it.
//
// Each site has a bit; the launchers fill their kernels' `wt` argument with wt_mask(): WT_DEFAULT, or IDELUCS_DEV=store_wt=<mask> (read at every
// launch: a captured graph keeps the mask it was captured with).  DESIGN.md 4.4 has the measurement behind WT_DEFAULT.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "dev_env.h"

namespace idl_store {

enum : int {
    WT_NEXT_PLANES = 1,     // A: the next batch's planes and its fp32 rows (scaler_device.h gather_tile: the riders and the stand-alone gathers)
    WT_PART = 2,            // B: layer 1's K-slice partial sums (l1_planes_device.h, both orientations)
    WT_W_V = 4,             // C: W1 and square_avg (wgrad_planes_device.h dplanes_body)
    WT_W_PLANES = 8,        // D: W1's planes (the same epilogue)
    WT_ALL = 15,
};
constexpr int WT_DEFAULT = WT_PART;      // (the sites that cleared the rule of tools/bench_store_policy.py: profiles/store_policy_ab.jsonl)

inline int wt_mask()
{
    const char *e = idl::dev_env("store_wt");
    return e != nullptr ? (int)strtol(e, nullptr, 0) & WT_ALL : WT_DEFAULT;
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// (no "memory" clobber: the sites read LDS images between their stores and must keep those reads in flight; see the head of the file for why none is needed.
//  s_nop 1: the store reads its data registers after issue, and the compiler does not pad behind an asm statement)
__device__ __forceinline__ void store16_wt(void *p, u32x4 v)
{
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(p), "v"(v));
}

template <class T>
__device__ __forceinline__ void store16(T *p, const T &v, bool wt)
{
    static_assert(sizeof(T) == 16, "store16: 16-byte values");
    if (wt) store16_wt(p, __builtin_bit_cast(u32x4, v));
    else *p = v;
}

// Two 8-byte stores a lane -> one 16-byte store a lane.  Lanes 2j and 2j + 1 hold (h, l) for adjacent groups of four elements of one row of two planes:
// they swap one uint2 (quad_perm [1, 0, 3, 2]), the even lane then holds 16 bytes of the first plane and the odd lane 16 bytes of the second, both
// at the even lane's element.  Every lane of a pair must be active.
__device__ __forceinline__ u32x4 pair_planes(uint2 h, uint2 l, bool odd)
{
    const uint32_t gx = odd ? h.x : l.x, gy = odd ? h.y : l.y;
    const uint32_t tx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)gx, 0xB1, 0xF, 0xF, false);
    const uint32_t ty = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)gy, 0xB1, 0xF, 0xF, false);
    u32x4 v;
    v.x = odd ? tx : h.x; v.y = odd ? ty : h.y; v.z = odd ? l.x : tx; v.w = odd ? l.y : ty;
    return v;
}

}  // namespace idl_store
