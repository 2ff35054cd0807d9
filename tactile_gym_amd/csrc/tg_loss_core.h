// tg_loss_core.h - what tg_loss_head.hip (PPO's loss) and tg_sac_loss.hip (SAC's losses) share: the sum of one
// chunk of 256 rows, one copy.  A workgroup is 256 lanes, one row per lane; every value is a double.  Inside each wave of 64 lanes the tree
// v[i] += v[i + off], off = 32 .. 1; lane 0 of each wave writes its wave's sum to LDS, and after a barrier the four wave sums are added in
// wave order.  The callers add the chunk sums in ascending order.  tests/loss_head_ref.py (tree_sum) restates it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace tg {

constexpr int kLossThreads = 256;                 // the chunk
constexpr int kLossWaves = kLossThreads / 64;

// Lane 0 of each wave: the sum of the wave's 64 values by the tree v[i] += v[i + off], off = 32, 16, 8, 4, 2, 1.
__device__ __forceinline__ double wave_sum(double v) {
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ void slot_put(double* lds, int slot, double v) {
    const double s = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[slot * kLossWaves + (threadIdx.x >> 6)] = s;
}

// The sum that thread `slot` owns, after a barrier: the wave sums in wave order.
__device__ __forceinline__ double slot_get(const double* lds, int slot) {
    return ((lds[slot * kLossWaves] + lds[slot * kLossWaves + 1]) + lds[slot * kLossWaves + 2]) + lds[slot * kLossWaves + 3];
}

}  // namespace tg
